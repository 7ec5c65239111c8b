"""Batched device decoder: Vorbis audio packets -> PCM for many streams sharing one set of headers, over the C ABI
of include/vorbis_mi355x.h (vbm_decode_setup_*, vbm_decoder_*, vbm_synthesis_batch).  Per row, one call does what
the reference's application loop does per packet: vorbis_synthesis + vorbis_synthesis_blockin +
vorbis_synthesis_pcmout + vorbis_synthesis_read (reference examples/decoder_example.c).  Every step from the packet
bytes to the PCM runs in gfx950 kernels; there is no CPU fallback."""
import ctypes as C

import numpy as np
import torch

from ._lib import lib, check

ENOTVORBIS, EBADHEADER, EVERSION, ENOTAUDIO, EBADPACKET = -132, -133, -134, -135, -136


class DecodeSetup:
    """The three header packets (vorbis_synthesis_headerin x3).  Host only: no device needed."""

    def __init__(self, headers):
        headers = [bytes(h) for h in headers]
        if len(headers) != 3:
            raise ValueError("need the three header packets")
        blob = b"".join(headers)
        lens = (C.c_long * 3)(*[len(h) for h in headers])
        buf = (C.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
        self._h = C.c_void_p()
        self.rc = lib.vbm_decode_setup_create(C.byref(self._h), buf, lens)
        check(self.rc, "vbm_decode_setup_create")
        ch, rate, bs, modes = C.c_int(), C.c_long(), (C.c_int * 2)(), C.c_int()
        check(lib.vbm_decode_setup_info(self._h, C.byref(ch), C.byref(rate), bs, C.byref(modes)), "vbm_decode_setup_info")
        self.channels, self.rate, self.blocksizes, self.modes = ch.value, rate.value, (bs[0], bs[1]), modes.value

    @staticmethod
    def status(headers):
        """return code of vbm_decode_setup_create for these headers (0 or a VBM_E* code), without raising"""
        blob = b"".join(bytes(h) for h in headers)
        lens = (C.c_long * 3)(*[len(bytes(h)) for h in headers])
        buf = (C.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
        h = C.c_void_p()
        rc = lib.vbm_decode_setup_create(C.byref(h), buf, lens)
        if rc == 0:
            lib.vbm_decode_setup_destroy(h)
        return rc

    def counts(self):
        """-> (books, floors, residues, mappings) of the setup header"""
        c = (C.c_int * 4)()
        check(lib.vbm_decode_setup_counts(self._h, c), "vbm_decode_setup_counts")
        return tuple(c)

    def unpack(self, packet):
        """Host instance of the device's packet unpack -> (status, info[4], floor_index [ch][bs1/2] int32,
        residue [ch][bs1/2] float32, floor_used [ch] int32)."""
        half = self.blocksizes[1] // 2
        info = (C.c_int * 4)()
        findex = np.zeros((self.channels, half), np.int32)
        res = np.zeros((self.channels, half), np.float32)
        used = np.zeros(self.channels, np.int32)
        pk = bytes(packet)
        buf = (C.c_ubyte * max(len(pk), 1)).from_buffer_copy(pk or b"\0")
        rc = lib.vbm_host_unpack_packet(self._h, buf, len(pk), info, findex.ctypes.data, res.ctypes.data,
                                        used.ctypes.data)
        return rc, list(info), findex, res, used

    def close(self):
        if self._h:
            lib.vbm_decode_setup_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Decoder:
    """nstreams decode streams on the current CUDA device; up to max_batch packets per call."""

    def __init__(self, dsetup, nstreams, max_batch):
        self.dsetup = dsetup
        self.channels, self.blocksizes = dsetup.channels, dsetup.blocksizes
        self.nstreams, self.max_batch = nstreams, max_batch
        self._h = C.c_void_p()
        check(lib.vbm_decoder_create(C.byref(self._h), dsetup._h, nstreams, max_batch), "vbm_decoder_create")
        self._last = None

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def synthesis_batch(self, stream_ids, packets, nbytes, granulepos=None, eos=None, out=None):
        """stream_ids: host ints (distinct); packets: uint8 [nsb, stride] and nbytes: int32 [nsb] on the device;
        granulepos: int64 [nsb] (-1: none) or None; eos: uint8 [nsb] or None.
        -> (pcm float32 [nsb, channels, blocksizes[1]//2], samples int32 [nsb], status int32 [nsb]), device tensors.
        Only enqueues work on the current stream."""
        ids = np.ascontiguousarray(np.asarray(stream_ids, dtype=np.int32))
        nsb = len(ids)
        dev = packets.device
        assert packets.dtype == torch.uint8 and packets.dim() == 2 and packets.is_contiguous()
        nbytes = nbytes.to(torch.int32).contiguous()
        if out is None:
            pcm = torch.empty((nsb, self.channels, self.blocksizes[1] // 2), dtype=torch.float32, device=dev)
            samples = torch.empty(nsb, dtype=torch.int32, device=dev)
            status = torch.empty(nsb, dtype=torch.int32, device=dev)
        else:
            pcm, samples, status = out
        gp = granulepos.to(torch.int64).contiguous() if granulepos is not None else None
        eo = eos.to(torch.uint8).contiguous() if eos is not None else None
        check(lib.vbm_synthesis_batch(self._h, nsb, ids.ctypes.data, packets.data_ptr(), packets.stride(0),
                                      nbytes.data_ptr(), gp.data_ptr() if gp is not None else None,
                                      eo.data_ptr() if eo is not None else None, pcm.data_ptr(), samples.data_ptr(),
                                      status.data_ptr(), self._stream()), "vbm_synthesis_batch")
        self._last = (nsb, dev, packets, nbytes, gp, eo)     # inputs stay alive until the work has run
        return pcm, samples, status

    def fetch(self, name):
        """Intermediate of the last call: "info" [nsb, 4], "floor_used" [nsb, ch], "floor_index" / "residue" /
        "spectrum" [nsb, ch, blocksizes[1]//2]."""
        nsb, dev = self._last[0], self._last[1]
        rows, kind = C.c_long(), C.c_char()
        st = self._stream()
        check(lib.vbm_decoder_fetch(self._h, name.encode(), None, C.byref(rows), C.byref(kind), st), "vbm_decoder_fetch")
        dt = torch.float32 if kind.value == b"f" else torch.int32
        if name == "info":
            shape = (nsb, 4)
        elif rows.value == 1:
            shape = (nsb, self.channels)
        else:
            shape = (nsb, self.channels, rows.value)
        out = torch.empty(shape, dtype=dt, device=dev)
        check(lib.vbm_decoder_fetch(self._h, name.encode(), out.data_ptr(), C.byref(rows), C.byref(kind), st),
              "vbm_decoder_fetch")
        return out

    def restart_streams(self, stream_ids):
        """vorbis_synthesis_restart for these streams (enqueued on the current stream)"""
        ids = np.ascontiguousarray(np.asarray(stream_ids, dtype=np.int32))
        check(lib.vbm_decoder_restart_streams(self._h, len(ids), ids.ctypes.data, self._stream()),
              "vbm_decoder_restart_streams")

    def reset(self):
        check(lib.vbm_decoder_reset(self._h), "vbm_decoder_reset")

    def close(self):
        if self._h:
            lib.vbm_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
