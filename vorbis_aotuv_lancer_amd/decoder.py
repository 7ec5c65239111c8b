"""Batched device decoder: Vorbis audio packets -> PCM for many streams sharing one set of headers, over the C ABI
of include/vorbis_mi355x.h (vbm_decode_setup_*, vbm_decoder_*, vbm_synthesis_batch).  Per row, one call does what
the reference's application loop does per packet: vorbis_synthesis + vorbis_synthesis_blockin +
vorbis_synthesis_pcmout + vorbis_synthesis_read (reference examples/decoder_example.c).  Every step from the packet
bytes to the PCM runs in gfx950 kernels; there is no CPU fallback."""
import ctypes as C

import numpy as np
import torch

from ._lib import lib, check, VbmError
from ._twin import _Handle, _TwinHandle, ptr, size

ENOTVORBIS, EBADHEADER, EVERSION, ENOTAUDIO, EBADPACKET = -132, -133, -134, -135, -136


def _i32(ints):
    """host ints (stream ids, counts, lengths) -> int32 [n], contiguous"""
    return np.ascontiguousarray(np.asarray(ints, dtype=np.int32))


def _per_packet(granulepos, eos, P=None):
    """The optional per-packet CUDA tensors -> (int64 or None, uint8 or None), contiguous; of P entries when P is given"""
    gp = granulepos.to(torch.int64).contiguous() if granulepos is not None else None
    eo = eos.to(torch.uint8).contiguous() if eos is not None else None
    if P is not None and ((gp is not None and gp.numel() != P) or (eo is not None and eo.numel() != P)):
        raise ValueError("granulepos and eos need one entry per packet")
    return gp, eo


def _csr_np(data, offsets, granulepos, eos):
    """A host CSR -> (data uint8, offsets int64, P, granulepos int64 [P] or None, eos uint8 [P] or None), contiguous"""
    data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
    offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    P = len(offsets) - 1
    if P < 0:
        raise ValueError("offsets needs at least one entry")
    gp = None if granulepos is None else np.ascontiguousarray(np.asarray(granulepos, dtype=np.int64))
    eo = None if eos is None else np.ascontiguousarray(np.asarray(eos, dtype=np.uint8))
    if (gp is not None and len(gp) != P) or (eo is not None and len(eo) != P):
        raise ValueError("granulepos and eos need one entry per packet")
    return data, offsets, P, gp, eo


def _csr_t(data, offsets, granulepos, eos, stream_packets):
    """A CSR in CUDA tensors -> (offsets int64, P, first int64 [S + 1] numpy, granulepos, eos as _per_packet's)"""
    assert data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
    offsets = offsets.to(torch.int64).contiguous()
    P = offsets.numel() - 1
    if P < 0:
        raise ValueError("offsets needs at least one entry")
    return (offsets, P, _stream_packets(stream_packets, P)) + _per_packet(granulepos, eos, P)


class DecodeSetup(_Handle):
    """The three header packets (vorbis_synthesis_headerin x3).  Host only: no device needed."""
    _destroy = "vbm_decode_setup_destroy"

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


class Decoder(_Handle):
    """nstreams decode streams on the current CUDA device; up to max_batch packets per call.
    halfrate=True (the reference's vorbis_synthesis_halfrate): the PCM comes out at dsetup.rate / 2, from inverse
    MDCTs of half each block size; every PCM row is blocksizes[1]//4 long instead of blocksizes[1]//2, and sample
    counts, range starts and lengths are output samples.  .rate is the output rate (an int when it is whole)."""
    _destroy = "vbm_decoder_destroy"

    def __init__(self, dsetup, nstreams, max_batch, halfrate=False):
        self.dsetup = dsetup
        self.channels, self.blocksizes = dsetup.channels, dsetup.blocksizes
        self.nstreams, self.max_batch = nstreams, max_batch
        self.halfrate = bool(halfrate)
        self.rate = output_rate(dsetup.rate, self.halfrate)
        self.row = dsetup.blocksizes[1] // (4 if self.halfrate else 2)      # most samples one packet returns
        self._h = C.c_void_p()
        check(lib.vbm_decoder_create_halfrate(C.byref(self._h), dsetup._h, nstreams, max_batch, int(self.halfrate)),
              "vbm_decoder_create_halfrate")
        self._last = None

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def synthesis_batch(self, stream_ids, packets, nbytes, granulepos=None, eos=None, out=None):
        """stream_ids: host ints (distinct); packets: uint8 [nsb, stride] and nbytes: int32 [nsb] on the device;
        granulepos: int64 [nsb] (-1: none) or None; eos: uint8 [nsb] or None.
        -> (pcm float32 [nsb, channels, blocksizes[1]//2], samples int32 [nsb], status int32 [nsb]), device tensors
        (blocksizes[1]//4 on a half-rate decoder).  Only enqueues work on the current stream."""
        ids = _i32(stream_ids)
        nsb = len(ids)
        dev = packets.device
        assert packets.dtype == torch.uint8 and packets.dim() == 2 and packets.is_contiguous()
        nbytes = nbytes.to(torch.int32).contiguous()
        if out is None:
            pcm = torch.empty((nsb, self.channels, self.row), dtype=torch.float32, device=dev)
            samples = torch.empty(nsb, dtype=torch.int32, device=dev)
            status = torch.empty(nsb, dtype=torch.int32, device=dev)
        else:
            pcm, samples, status = out
        gp, eo = _per_packet(granulepos, eos)
        check(lib.vbm_synthesis_batch(self._h, nsb, ids.ctypes.data, packets.data_ptr(), packets.stride(0),
                                      nbytes.data_ptr(), ptr(gp), ptr(eo), pcm.data_ptr(), samples.data_ptr(),
                                      status.data_ptr(), self._stream()), "vbm_synthesis_batch")
        self._last = (nsb, dev, packets, nbytes, gp, eo)     # inputs stay alive until the work has run
        return pcm, samples, status

    def synthesis_runs(self, stream_ids, counts, data, offsets, granulepos=None, eos=None, pcm_stride=None, out=None,
                       gap=None):
        """Many packets per stream: run r is counts[r] consecutive packets of stream stream_ids[r] (host ints; ids
        distinct), rows are the runs concatenated (P = sum(counts) <= max_batch).  data: uint8 [bytes] and offsets:
        int64 [P+1] on the device (CSR: packet k is data[offsets[k]:offsets[k+1]]); granulepos int64 [P] / eos uint8
        [P] or None.  gap: uint8 [P] on the device or None (FeedResult.gap of a resync OggFeed): a non-zero mark says
        packets were lost in front of that packet, and the stream's granule position and sample count start over there
        (the overlap-add goes on).  pcm_stride defaults to max(counts) * blocksizes[1]//2 (//4 on a half-rate decoder).
        -> (pcm float32 [nruns, channels, pcm_stride], run_samples int32 [nruns], samples int32 [P],
        status int32 [P]), device tensors; run r's PCM is pcm[r, :, :run_samples[r]].  Bit-identical to one packet per
        call through synthesis_batch.  Only enqueues work on the current stream."""
        ids, cnt = _i32(stream_ids), _i32(counts)
        if ids.shape != cnt.shape or ids.ndim != 1:
            raise ValueError("stream_ids and counts must be 1-D and of the same length")
        nruns, P = len(ids), int(cnt.sum())
        dev = offsets.device
        assert data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
        offsets = offsets.to(torch.int64).contiguous()
        if offsets.numel() != P + 1:
            raise ValueError(f"offsets must have sum(counts) + 1 = {P + 1} entries, has {offsets.numel()}")
        if pcm_stride is None:
            pcm_stride = self._run_stride(ids, cnt)
        if out is None:
            pcm = torch.empty((nruns, self.channels, pcm_stride), dtype=torch.float32, device=dev)
            run_samples = torch.empty(nruns, dtype=torch.int32, device=dev)
            samples = torch.empty(P, dtype=torch.int32, device=dev)
            status = torch.empty(P, dtype=torch.int32, device=dev)
        else:
            pcm, run_samples, samples, status = out
            pcm_stride = pcm.stride(1)
        gp, eo = _per_packet(granulepos, eos)
        if gap is not None:
            gap = gap.to(torch.uint8).contiguous()
            if gap.numel() != P:
                raise ValueError(f"gap must have sum(counts) = {P} entries, has {gap.numel()}")
        check(lib.vbm_synthesis_runs_gaps(self._h, nruns, ids.ctypes.data, cnt.ctypes.data, data.data_ptr(),
                                          offsets.data_ptr(), data.numel(), ptr(gp), ptr(eo), ptr(gap), pcm.data_ptr(),
                                          pcm_stride, run_samples.data_ptr(), samples.data_ptr(), status.data_ptr(),
                                          self._stream()), "vbm_synthesis_runs_gaps")
        if P:
            self._last = (P, dev, data, offsets, gp, eo, gap)  # inputs stay alive until the work has run
        return pcm, run_samples, samples, status

    def synthesis_ranges(self, store, stream_ids, starts, lengths, pcm_stride=None, out=None):
        """Sample windows of a RangeStore's streams: range r is lengths[r] samples of stream stream_ids[r] from sample
        starts[r] of its linear decode (host ints).  pcm_stride defaults to max(lengths).
        -> (pcm float32 [n, channels, pcm_stride] on the device, got int32 [n] numpy), pcm[r, :, :got[r]] bit for bit
        the linear decode's samples; nothing else of pcm is written.  Reads and writes no stream state; only
        enqueues work on the current stream."""
        ids, ln = _i32(stream_ids), _i32(lengths)
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int64))
        if not (ids.ndim == st.ndim == ln.ndim == 1 and len(ids) == len(st) == len(ln)):
            raise ValueError("stream_ids, starts and lengths must be 1-D and of the same length")
        n = len(ids)
        if pcm_stride is None:
            pcm_stride = max(1, int(ln.max(initial=0)))
        if out is None:
            pcm = torch.empty((n, self.channels, pcm_stride), dtype=torch.float32,
                              device=torch.device("cuda", torch.cuda.current_device()))
        else:
            pcm = out
            pcm_stride = pcm.stride(1)
        got = np.zeros(n, np.int32)
        check(lib.vbm_synthesis_ranges(self._h, store._h, n, ids.ctypes.data, st.ctypes.data, ln.ctypes.data,
                                       pcm.data_ptr(), pcm_stride, got.ctypes.data, self._stream()),
              "vbm_synthesis_ranges")
        return pcm, got

    def fetch(self, name):
        """Intermediate of the last call: "info" [nsb, 4], "floor_used" [nsb, ch], "floor_index" / "residue" /
        "spectrum" [nsb, ch, blocksizes[1]//2] (the full-rate intermediates on a half-rate decoder too)."""
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
        ids = _i32(stream_ids)
        check(lib.vbm_decoder_restart_streams(self._h, len(ids), ids.ctypes.data, self._stream()),
              "vbm_decoder_restart_streams")

    def reset(self):
        check(lib.vbm_decoder_reset(self._h), "vbm_decoder_reset")

    def _hold_index_inputs(self, *tensors):
        """decode_index_device's inputs stay alive until the work has run (apart from ._last, which fetch reads)"""
        self._last_index = tensors

    def _run_stride(self, ids, counts):
        """synthesis_runs' default pcm_stride: room for the longest run"""
        return max(1, int(counts.max(initial=0)) * self.row)


class MixedDecoder(Decoder):
    """A Decoder for streams of different header classes (vbm_decoder_create_mixed): made from caps instead of a
    setup, up to max_classes classes of up to max_channels channels and blocks of up to max_blocksize.
        c = md.add_class(dsetup)            # or md.class_for(headers): adds, or finds by byte-equal headers
        md.bind(stream_ids, class_ids)      # also restarts those streams
    synthesis_batch and synthesis_runs then take streams of any mix of classes in one call and one launch chain, each
    stream's result bit for bit that of a Decoder of its class.  Their PCM rows are the caps': pcm is [n, max_channels,
    stride], and row r uses pcm[r, :channels_of([id])[0], :samples]; the rest is not written.  A call that lists an
    unbound stream is a VbmError.  .channels is max_channels and .row the most samples a packet of the largest block
    returns; rates and channel counts are per stream: rate_of(ids), channels_of(ids).
    Random access: RangeStore(md, streams, classes=[class id per stream]) (and RangeStore.from_device,
    decode_index_device with classes=) keeps streams of any mix of classes; the store's classes are its own, not bind's.
    synthesis_ranges(store, ids, starts, lengths) then returns pcm [n, max_channels, stride], of which range r uses
    the channels of its stream's class and got[r] samples; the rest is not written.  One launch chain per sub-call,
    whatever the classes.  fetch is not built for it (VbmError)."""

    def __init__(self, nstreams, max_batch, max_classes=64, max_channels=8, max_blocksize=4096, halfrate=False):
        self.dsetup, self.blocksizes, self.rate = None, None, None
        self.channels, self.max_classes, self.max_blocksize = max_channels, max_classes, max_blocksize
        self.nstreams, self.max_batch = nstreams, max_batch
        self.halfrate = bool(halfrate)
        self.row = max_blocksize // (4 if self.halfrate else 2)
        self._h = C.c_void_p()
        check(lib.vbm_decoder_create_mixed(C.byref(self._h), max_classes, max_channels, max_blocksize, nstreams,
                                           max_batch, int(self.halfrate)), "vbm_decoder_create_mixed")
        self._last = None
        self.classes = []                                     # DecodeSetup of every class, by class id
        self._by_headers = {}                                 # (identification, setup packet) -> class id
        self._own = []                                        # the setups class_for made: closed with the decoder
        self.stream_class = np.full(nstreams, -1, np.int32)   # the host mirror of the binding

    def add_class(self, dsetup):
        """-> the class id (0, 1, ...) of this DecodeSetup, copied to the device on the current stream.  The setup must
        stay open as long as the decoder uses it for channels_of / rate_of."""
        cid = C.c_int(-1)
        check(lib.vbm_decoder_add_class(self._h, dsetup._h, C.byref(cid), self._stream()), "vbm_decoder_add_class")
        assert cid.value == len(self.classes)
        self.classes.append(dsetup)
        return cid.value

    def class_for(self, headers):
        """-> the class id of these three header packets: the class with byte-equal identification and setup packets,
        added if it is new"""
        key = (bytes(headers[0]), bytes(headers[2]))
        if key not in self._by_headers:
            ds = DecodeSetup(headers)
            try:
                self._by_headers[key] = self.add_class(ds)
            except VbmError:
                ds.close()
                raise
            self._own.append(ds)
        return self._by_headers[key]

    def bind(self, stream_ids, class_ids):
        """streams stream_ids (distinct) are of classes class_ids from here on, and restart (enqueued on the current
        stream, in order with the calls around it)"""
        ids, cls = _i32(stream_ids), _i32(class_ids)
        if ids.shape != cls.shape or ids.ndim != 1:
            raise ValueError("stream_ids and class_ids must be 1-D and of the same length")
        check(lib.vbm_decoder_bind_streams(self._h, len(ids), ids.ctypes.data, cls.ctypes.data, self._stream()),
              "vbm_decoder_bind_streams")
        self.stream_class[ids] = cls

    def _of(self, ids, what):
        cls = self.stream_class[_i32(ids)]
        if (cls < 0).any():
            raise ValueError("a stream is not bound to a class")
        return [what(self.classes[c]) for c in cls]

    def channels_of(self, ids):
        """the channel count of each of these streams' classes"""
        return self._of(ids, lambda ds: ds.channels)

    def rate_of(self, ids):
        """the output rate of each of these streams (half the class's on a half-rate decoder)"""
        return self._of(ids, lambda ds: output_rate(ds.rate, self.halfrate))

    def row_of(self, ids):
        """the most samples one packet of each of these streams returns"""
        return self._of(ids, lambda ds: ds.blocksizes[1] // (4 if self.halfrate else 2))

    def fetch(self, name):
        """not built for a mixed decoder: the VbmError of vbm_decoder_fetch"""
        check(lib.vbm_decoder_fetch(self._h, name.encode(), None, None, None, self._stream()), "vbm_decoder_fetch")

    def _run_stride(self, ids, counts):
        # a stream id out of range or unbound is left out here: the call itself refuses it with its VbmError
        bound = (ids >= 0) & (ids < self.nstreams)
        bound[bound] = self.stream_class[ids[bound]] >= 0
        rows = np.asarray(self.row_of(ids[bound]), dtype=np.int64)
        return max(1, int((counts[bound] * rows).max(initial=0)))

    def close(self):
        super().close()
        for ds in self._own:
            ds.close()
        self._own = []


def output_rate(rate, halfrate):
    """the rate of a decoder's PCM: rate, or rate / 2 at half rate (a float only when rate is odd)"""
    if not halfrate:
        return rate
    return rate // 2 if rate % 2 == 0 else rate / 2


def decode_index(dsetup, data, offsets, granulepos=None, eos=None, halfrate=False):
    """Host index of one stream's demuxed packets (vbm_decode_index_halfrate; no device needed): data uint8 [bytes],
    offsets int64 [P+1], granulepos int64 [P], eos uint8 [P] (numpy, as demux_ogg returns them).  halfrate: the index
    of a Decoder(..., halfrate=True), in its output samples.
    -> (status int32 [P], samples int32 [P], out_start int64 [P], total)"""
    data, offsets, P, gp, eo = _csr_np(data, offsets, granulepos, eos)
    status, samples = np.zeros(P, np.int32), np.zeros(P, np.int32)
    out_start = np.zeros(P, np.int64)
    total = C.c_longlong()
    check(lib.vbm_decode_index_halfrate(dsetup._h, int(bool(halfrate)), P, ptr(data, len(data)), offsets.ctypes.data,
                                        len(data), ptr(gp), ptr(eo), status.ctypes.data, samples.ctypes.data,
                                        out_start.ctypes.data, C.byref(total)), "vbm_decode_index_halfrate")
    return status, samples, out_start, total.value


def _stream_packets(stream_packets, P):
    """None: one stream of P packets -> int64 [S + 1], contiguous"""
    first = np.asarray([0, P] if stream_packets is None else stream_packets, dtype=np.int64)
    if first.ndim != 1 or len(first) < 2 or int(first[-1]) != P:
        raise ValueError(f"stream_packets must run from 0 to the packet count {P} (one entry per stream, and one)")
    return np.ascontiguousarray(first)


def _stream_classes(classes, nstreams):
    """None, or one class id per stream -> int32 [nstreams], contiguous"""
    if classes is None:
        return None
    cls = _i32(classes)
    if cls.ndim != 1 or len(cls) != nstreams:
        raise ValueError(f"classes needs one class id per stream: {nstreams}, has {cls.size}")
    return cls


def decode_index_device(decoder, data, offsets, granulepos=None, eos=None, stream_packets=None, classes=None):
    """The index of demuxed streams, built on the device (vbm_decode_index_device) at the decoder's rate: data uint8
    [bytes], offsets int64 [P+1], granulepos int64 [P] / eos uint8 [P] or None, CUDA tensors holding one CSR over the
    packets of all streams (a DemuxBatch's payload, offsets, granulepos and eos); stream_packets: host ints [S+1], the
    first packet of every stream and P (None: one stream).
    -> (status int32 [P], begin int32 [P], end int32 [P], out_start int64 [P], totals int64 [S]), device tensors;
    end - begin, out_start and totals are decode_index's samples, out_start and total of each stream alone.  Only
    enqueues work on the current stream.  classes: with a MixedDecoder, the class id of every stream (required;
    vbm_decode_index_device_mixed): each stream's index is that of its own class.  With a Decoder it is an error."""
    offsets, P, first, gp, eo = _csr_t(data, offsets, granulepos, eos, stream_packets)
    cls = _stream_classes(classes, len(first) - 1)
    dev = offsets.device
    status, begin, end = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    out_start = torch.empty(P, dtype=torch.int64, device=dev)
    totals = torch.empty(len(first) - 1, dtype=torch.int64, device=dev)
    name, extra = ("vbm_decode_index_device", ()) if cls is None else ("vbm_decode_index_device_mixed", (cls.ctypes.data,))
    check(getattr(lib, name)(decoder._h, len(first) - 1, first.ctypes.data, *extra, ptr(data, data.numel()),
                             offsets.data_ptr(), data.numel(), ptr(gp, P), ptr(eo, P), status.data_ptr(),
                             begin.data_ptr(), end.data_ptr(), out_start.data_ptr(), totals.data_ptr(),
                             decoder._stream()), name)
    decoder._hold_index_inputs(data, offsets, gp, eo)
    return status, begin, end, out_start, totals


def decode_index_scan_host(dsetup, data, offsets, granulepos=None, eos=None, stream_packets=None, halfrate=False,
                           classes=None):
    """The CPU twin of decode_index_device (vbm_host_decode_index_scan; no device needed), on numpy arrays.
    classes: dsetup is then a list of DecodeSetups and classes the index into it of every stream
    (vbm_host_decode_index_scan_mixed, the twin of the index on a MixedDecoder).
    -> (status int32 [P], begin int32 [P], end int32 [P], out_start int64 [P], totals int64 [S])"""
    data, offsets, P, gp, eo = _csr_np(data, offsets, granulepos, eos)
    first = _stream_packets(stream_packets, P)
    status, begin, end = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    out_start, totals = np.zeros(P, np.int64), np.zeros(len(first) - 1, np.int64)
    if classes is not None:
        cls = _stream_classes(classes, len(first) - 1)
        setups = (C.c_void_p * max(len(dsetup), 1))(*[ds._h.value for ds in dsetup])
        check(lib.vbm_host_decode_index_scan_mixed(len(dsetup), setups, int(bool(halfrate)), len(first) - 1,
                                                   first.ctypes.data, cls.ctypes.data, ptr(data, len(data)),
                                                   offsets.ctypes.data, len(data), ptr(gp), ptr(eo),
                                                   status.ctypes.data, begin.ctypes.data, end.ctypes.data,
                                                   out_start.ctypes.data, totals.ctypes.data),
              "vbm_host_decode_index_scan_mixed")
        return status, begin, end, out_start, totals
    check(lib.vbm_host_decode_index_scan(dsetup._h, int(bool(halfrate)), len(first) - 1, first.ctypes.data,
                                         ptr(data, len(data)), offsets.ctypes.data, len(data), ptr(gp), ptr(eo),
                                         status.ctypes.data, begin.ctypes.data, end.ctypes.data, out_start.ctypes.data,
                                         totals.ctypes.data), "vbm_host_decode_index_scan")
    return status, begin, end, out_start, totals


class RangeStore(_Handle):
    """The packets of many streams of one Decoder's headers in device memory, with their index, for
    Decoder.synthesis_ranges.  streams: (data, offsets, granulepos, eos) tuples as demux_ogg returns them (granulepos
    / eos may be None).  .totals: int64 [nstreams], each stream's linear decode length (ov_pcm_total), at the
    decoder's rate: .halfrate is the decoder's.  classes: with a MixedDecoder, the class id of every stream (required;
    the streams may then be of any mix of the decoder's classes, and .classes keeps them); with a Decoder an error."""
    _destroy = "vbm_range_store_destroy"

    def __init__(self, decoder, streams, classes=None):
        streams = list(streams)
        if not streams:
            raise ValueError("a range store needs at least one stream")
        cls = _stream_classes(classes, len(streams))
        datas, offs, gps, eoss, first, base = [], [np.zeros(1, np.int64)], [], [], [0], 0
        for data, o, gp, eo in streams:
            data = np.asarray(data, dtype=np.uint8).ravel()
            o = np.asarray(o, dtype=np.int64)
            P = len(o) - 1
            datas.append(data)
            offs.append(o[1:] + base)
            gps.append(np.full(P, -1, np.int64) if gp is None else np.asarray(gp, dtype=np.int64))
            eoss.append(np.zeros(P, np.uint8) if eo is None else np.asarray(eo, dtype=np.uint8))
            first.append(first[-1] + P)
            base += len(data)
        data = np.ascontiguousarray(np.concatenate(datas)) if datas else np.zeros(0, np.uint8)
        offsets = np.ascontiguousarray(np.concatenate(offs))
        gp = np.ascontiguousarray(np.concatenate(gps))
        eo = np.ascontiguousarray(np.concatenate(eoss))
        self._create(decoder, np.ascontiguousarray(np.asarray(first, np.int64)), cls, "vbm_range_store_create",
                     ptr(data, len(data)), offsets.ctypes.data, len(data), gp.ctypes.data, eo.ctypes.data)

    def _create(self, decoder, first, cls, create, *csr):
        """the tail of both constructors: the fields, the C store from create(..., stream_packets, *csr), or with the
        streams' classes from create_mixed(..., stream_packets, classes, *csr); its totals"""
        self.decoder, self.nstreams, self.halfrate = decoder, len(first) - 1, decoder.halfrate
        self.packets, self.classes = first, cls
        self._h = C.c_void_p()
        if cls is not None:
            create, csr = create + "_mixed", (cls.ctypes.data,) + csr
        check(getattr(lib, create)(C.byref(self._h), decoder._h, self.nstreams, first.ctypes.data, *csr), create)
        self.totals = np.zeros(self.nstreams, np.int64)
        check(lib.vbm_range_store_totals(self._h, self.totals.ctypes.data), "vbm_range_store_totals")

    @classmethod
    def from_device(cls, decoder, payload, offsets=None, granulepos=None, eos=None, stream_packets=None, classes=None):
        """The same store from a CSR that is already on the device (vbm_range_store_create_device): payload uint8
        [bytes], offsets int64 [P+1], granulepos int64 [P] / eos uint8 [P] or None as CUDA tensors, stream_packets host
        ints [S+1] (the first packet of every stream, and P).  A stream.DemuxBatch may be given in place of payload,
        alone: every file of it is a stream (a failed file an empty one).  The index is built by device kernels and
        no packet byte crosses to the host; the store keeps its own copies, so the tensors are free when this
        returns.  Waits for the device once.  classes: as the constructor's."""
        if offsets is None:
            b = payload
            payload, offsets, granulepos, eos = b.payload, b.offsets, b.granulepos, b.eos
            stream_packets = np.append(np.asarray(b.packet_base, dtype=np.int64), offsets.numel() - 1)
        if offsets.numel() < 1 or stream_packets is None:
            raise ValueError("offsets needs at least one entry, and stream_packets must be given")
        offsets, P, first, gp, eo = _csr_t(payload, offsets, granulepos, eos, stream_packets)
        self = cls.__new__(cls)
        self._create(decoder, first, _stream_classes(classes, len(first) - 1), "vbm_range_store_create_device",
                     ptr(payload, payload.numel()),
                     offsets.data_ptr(), payload.numel(), ptr(gp, P), ptr(eo, P), decoder._stream())
        return self


LIVE_EBIG = -1004


class LiveAppend:
    """What LiveRangeStore.append did, per entry: status (0, LIVE_EBIG: the run is larger than a capacity and the slot
    was left as it was, or VBM_EINVAL -131: its offsets are no CSR), dropped (packets that left the slot's front) and
    retained (packets the slot holds now), int32 numpy arrays"""

    def __init__(self, status, dropped, retained):
        self.status, self.dropped, self.retained = status, dropped, retained


class LiveRangeStore(RangeStore, _TwinHandle):
    """A time-shift buffer (vbm_live_store_*; csrc/live_store.h): a RangeStore with a fixed region per stream, max_packets
    packet slots and max_bytes payload bytes in device memory, that takes appended runs of packets and drops the oldest
    when a region is full.  Decoder.synthesis_ranges, MixedDecoder.synthesis_ranges and OggCutter.cut take it as they
    take a RangeStore.  Positions are output samples since the slot's last restart at the decoder's rate: the
    concatenation of what synthesis_runs returns for the same packets, granulepos, eos and gap in the same order.
    .totals [nstreams] is its end and .first_sample [nstreams] the first sample a window may start at (out_end of the
    first retained valid packet, which is only pre-roll); a window that starts earlier gets got = 0, a cut an empty file.
    decoder_or_setup: a Decoder or MixedDecoder; or, with host=True, a DecodeSetup: the CPU twin over numpy arrays, which
    needs no device (halfrate is then the twin's own; a device store has its decoder's).  A store of a MixedDecoder gives
    every slot its class with restart(ids, classes).  Calls on one store are ordered by the caller on one stream."""

    def __init__(self, decoder_or_setup, nstreams, max_packets, max_bytes, host=False, halfrate=False):
        self.host = bool(host)
        self.nstreams, self.max_packets, self.max_bytes = int(nstreams), int(max_packets), int(max_bytes)
        self._h = C.c_void_p()
        # the two forms are made from different things: the host twin from a setup and its own rate, the device form
        # from a decoder, plain or mixed
        if self.host:
            self.decoder, self.halfrate, self.classes = None, bool(halfrate), None
            check(lib.vbm_host_live_store_create(C.byref(self._h), decoder_or_setup._h, int(self.halfrate), self.nstreams,
                                                 self.max_packets, self.max_bytes), "vbm_host_live_store_create")
        else:
            self.decoder, self.halfrate = decoder_or_setup, decoder_or_setup.halfrate
            mixed = isinstance(decoder_or_setup, MixedDecoder)
            self.classes = np.full(self.nstreams, -1, np.int32) if mixed else None
            create = "vbm_live_store_create_mixed" if mixed else "vbm_live_store_create"
            check(getattr(lib, create)(C.byref(self._h), decoder_or_setup._h, self.nstreams, self.max_packets,
                                       self.max_bytes), create)
        self._refresh()

    def _q(self):
        """the decoder's stream; None for the host twin"""
        return None if self.host else self.decoder._stream()

    def _refresh(self):
        """.first_sample, .totals, .packets, .bytes, .stats from the store's host mirror"""
        S = self.nstreams
        self.first_sample, self.totals = np.zeros(S, np.int64), np.zeros(S, np.int64)
        self.packets, self.bytes = np.zeros(S, np.int64), np.zeros(S, np.int64)
        trims = np.zeros(2, np.int64)
        self._call("live_store_state", self.first_sample.ctypes.data, self.totals.ctypes.data, self.packets.ctypes.data,
                   self.bytes.ctypes.data, trims.ctypes.data)
        self.stats = {"trims_by_packets": int(trims[0]), "trims_by_bytes": int(trims[1])}

    def append(self, ids, counts, data, offsets, granulepos=None, eos=None, gap=None):
        """synthesis_runs' arguments: entry e is counts[e] consecutive packets for slot ids[e] (host ints, ids distinct,
        zero counts allowed), data uint8 [bytes] and offsets int64 [P + 1] one CSR over the packets of all entries in list
        order, granulepos int64 [P] / eos uint8 [P] / gap uint8 [P] or None: CUDA tensors (numpy arrays with host=True).
        The index goes on from each slot's carried state, so how a stream is split over appends does not show.  A run
        that does not fit makes its slot drop, from the front, the fewest packets such that what remains is at most half
        of each capacity and leaves room for the run.  Waits for the device once; the tensors are free when it returns.
        -> LiveAppend"""
        ids, cnt = _i32(ids), _i32(counts)
        if ids.shape != cnt.shape or ids.ndim != 1:
            raise ValueError("ids and counts must be 1-D and of the same length")
        n, P = len(ids), int(cnt.clip(min=0).sum())
        if self.host:
            data, offsets, _, gp, eo = _csr_np(data, offsets, granulepos, eos)
            gap = None if gap is None else np.ascontiguousarray(np.asarray(gap, dtype=np.uint8))
        else:
            assert data.dtype == torch.uint8 and data.dim() == 1 and data.is_contiguous()
            offsets = offsets.to(torch.int64).contiguous()
            gp, eo = _per_packet(granulepos, eos)
            gap = None if gap is None else gap.to(torch.uint8).contiguous()
        if size(offsets) != P + 1:
            raise ValueError(f"offsets must have sum(counts) + 1 = {P + 1} entries, has {size(offsets)}")
        for a in (gp, eo, gap):
            if a is not None and size(a) != P:
                raise ValueError("granulepos, eos and gap need one entry per packet")
        status, dropped, retained = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._call("live_store_append", n, ids.ctypes.data, cnt.ctypes.data, ptr(data, size(data)), ptr(offsets), size(data),
                   ptr(gp), ptr(eo), ptr(gap), status.ctypes.data, dropped.ctypes.data, retained.ctypes.data)
        self._refresh()
        return LiveAppend(status, dropped, retained)

    def restart(self, ids, classes=None):
        """The slots ids (distinct) are empty and fresh: positions start over at 0.  classes: with a store of a
        MixedDecoder, the class of each from here to its next restart (required); else an error.  Only enqueues."""
        ids = _i32(ids)
        # the two forms differ in more than the stream here: only the device form takes classes (and behind them its
        # stream, which _call adds only behind a twin's own arguments)
        if self.host:
            if classes is not None:
                raise ValueError("the host twin has one setup: no classes")
            self._call("live_store_restart", len(ids), ids.ctypes.data)
        else:
            cls = None if classes is None else _i32(classes)
            if cls is not None and cls.shape != ids.shape:
                raise ValueError("classes needs one class id per slot")
            self._call("live_store_restart", len(ids), ids.ctypes.data, ptr(cls), self._q())
            if cls is not None and self.classes is not None:
                self.classes[ids] = cls
        self._refresh()

    def snapshot(self):
        """The retained packets of all streams as a compact index and CSR in numpy arrays, the tuple
        OggCutter(host=True).cut takes: (first int64 [S + 1], status int32 [P], begin int32 [P], out_end int64 [P],
        totals int64 [S], data uint8, offsets int64 [P + 1]); positions stay absolute.  Waits for the device."""
        S, P, B = self.nstreams, int(self.packets.sum()), int(self.bytes.sum())
        first, totals, offsets = np.zeros(S + 1, np.int64), np.zeros(S, np.int64), np.zeros(P + 1, np.int64)
        status, begin, out_end = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int64)
        data = np.zeros(B, np.uint8)
        self._call("live_store_snapshot", first.ctypes.data, ptr(status, P), ptr(begin, P), ptr(out_end, P),
                   totals.ctypes.data, ptr(data, B), offsets.ctypes.data)
        return first, status, begin, out_end, totals, data, offsets


def _demux_host(name, blob):
    """demux_ogg of one file or link as an Entry (no gap marks), its errors under the entry's name"""
    from .stream import Entry, demux_ogg
    try:
        return Entry(*demux_ogg(blob), None)
    except VbmError as e:
        raise VbmError(f"{name}: {e}") from None


NO_VORBIS = "no Vorbis stream was found among its pages"


def _select_host(name, blob):
    """select_vorbis_stream of one file, the Vorbis stream's pages alone; VbmError under the file's name without one"""
    from .stream import select_vorbis_stream
    out = select_vorbis_stream(blob)
    if not out:                                           # the chosen page is kept: nothing kept, nothing chosen
        raise VbmError(f"{name}: {NO_VORBIS}")
    return out


def _raise_failed(batch, names):
    """VbmError for the first failed entry of a device-demuxed batch"""
    for i, (name, code) in enumerate(zip(names, batch.status)):
        if code:
            if batch.select_info is not None:
                f = int(np.searchsorted(batch.file_links, i, side="right")) - 1    # the given file of entry i
                if batch.select_info["streams"][f] == 0:
                    raise VbmError(f"{name}: {NO_VORBIS} (vbm_ogg_demux_scan failed with code {code} on the empty entry)")
            raise VbmError(f"{name}: vbm_ogg_demux_scan failed with code {code}: not one valid logical Ogg stream "
                           "(vbm_ogg_demux on the file alone names the page)")


def header_classes(headers):
    """Per-file header triples -> (class id of every file, the first file of every class, max channels, max block
    size): files are of one class when their identification and setup packets are byte-equal, and classes are numbered
    in order of first appearance.  The caps are read from the identification packets (channels: byte 11, the two block
    size exponents: byte 28).  Pure host code: no library call, no device."""
    ids, firsts, by = [], [], {}
    for i, h in enumerate(headers):
        key = (bytes(h[0]), bytes(h[2]))
        if key not in by:
            by[key] = len(firsts)
            firsts.append(i)
        ids.append(by[key])
    idents = [bytes(headers[i][0]) for i in firsts]
    for i, ident in zip(firsts, idents):
        if len(ident) < 30 or ident[:7] != b"\x01vorbis":
            raise ValueError(f"file {i}: not a Vorbis identification header")
    return ids, firsts, max(x[11] for x in idents), max(1 << (x[28] >> 4) for x in idents)


class OggIndex:
    """Random sample windows of many .ogg files (bytes or paths, one logical stream each, one set of headers: files
    whose identification or setup headers differ are a ValueError).  The files' packets and index stay in device
    memory (about the compressed size + 24 B per packet); no PCM is kept.  .total_samples: int64 [files].
    decode_ranges(file_ids, starts, lengths) -> (pcm float32 [n, channels, max(lengths)] CUDA tensor, zeros past got;
    got int32 [n]), pcm[r, :, :got[r]] bit for bit decode_ogg's output of that file from starts[r].
    cut_ranges(file_ids, starts, lengths) -> the same windows as new .ogg files, the packets copied unchanged.
    halfrate=True: .rate is half the files' rate, and total_samples, starts and lengths are samples at that rate
    (decode_ogg(files, halfrate=True)'s).  device_demux=True: the files are demuxed together on the device
    (stream.demux_ogg_device) and the store and its index are built there from the demuxed batch
    (RangeStore.from_device) instead of file by file on the host; the index and every range are the same bit for
    bit.  multiplexed=True: the files may carry other streams beside the Vorbis one (stream.StreamSelector on the
    device with device_demux, stream.select_vorbis_stream on the host without); a file without a Vorbis stream is a
    VbmError that says so.
    one_decoder=True (as decode_ogg's): the files may be of any mix of header classes.  They are grouped by byte-equal
    identification and setup headers (header_classes) and indexed in one store of one MixedDecoder, its caps the
    largest channel count and block size among them; decode_ranges returns [n, max channels, L], range r in the
    channels of its file and zeros elsewhere, and every clip of cut_ranges opens with its own file's header pages.
    .file_channels and .file_rates: one entry per file (on every index).  With one_decoder, .channels is the largest
    channel count, .rate the common output rate or None when the files' rates differ, and .setup is None (.setups:
    one per class, .file_class: the class of every file)."""

    def __init__(self, files, max_batch=4096, halfrate=False, device_demux=False, multiplexed=False,
                 one_decoder=False):
        from .stream import _read_files, demux_ogg_device
        if max_batch < 2:
            raise ValueError("max_batch must be at least 2")
        names, blobs = _read_files(files)
        if not blobs:
            raise ValueError("OggIndex needs at least one file")
        if device_demux:
            b = demux_ogg_device(blobs, multiplexed=multiplexed)
            _raise_failed(b, names)
        else:
            demuxed = [_demux_host(name, _select_host(name, blob) if multiplexed else blob)
                       for name, blob in zip(names, blobs)]
        headers = b.headers if device_demux else [d.headers for d in demuxed]
        classes = self._open_mixed(names, headers, max_batch, halfrate) if one_decoder else None
        if not one_decoder:
            self._open(headers, max_batch, halfrate)
        self.store = (RangeStore.from_device(self.decoder, b, classes=classes) if device_demux
                      else RangeStore(self.decoder, [(d.data, d.offsets, d.granulepos, d.eos) for d in demuxed], classes=classes))
        self.total_samples = self.store.totals

    def _open_mixed(self, names, headers, max_batch, halfrate):
        """any header classes -> .setups, .decoder (a MixedDecoder of their caps), the class of every file"""
        cls, firsts, max_ch, max_bs = header_classes(headers)
        for i in firsts:                                      # every setup is checked before any work is enqueued
            rc = DecodeSetup.status(headers[i])
            if rc:
                raise VbmError(f"{names[i]}: unsupported or invalid Vorbis headers (code {rc}): "
                               f"{lib.vbm_last_error().decode()}")
        self.setup, self.setups = None, [DecodeSetup(headers[i]) for i in firsts]
        self.decoder = MixedDecoder(1, max_batch, max_classes=len(firsts), max_channels=max_ch, max_blocksize=max_bs,
                                    halfrate=halfrate)
        for ds in self.setups:
            self.decoder.add_class(ds)
        self.halfrate = self.decoder.halfrate
        self.file_class = np.asarray(cls, dtype=np.int32)
        self.file_channels = np.asarray([self.setups[c].channels for c in cls], dtype=np.int64)
        self.file_rates = np.asarray([output_rate(self.setups[c].rate, self.halfrate) for c in cls])
        self.channels = int(self.file_channels.max())
        self.rate = self.file_rates[0].item() if (self.file_rates == self.file_rates[0]).all() else None
        self.headers = [[bytes(p) for p in h] for h in headers]
        self._hdr_pages, self._cutter = {}, None
        return cls

    def _open(self, headers, max_batch, halfrate):
        """one header class -> .setup, .decoder"""
        h0 = headers[0]
        for i, h in enumerate(headers):
            if h[0] != h0[0] or h[2] != h0[2]:
                raise ValueError(f"file {i} has other identification or setup headers than file 0: one OggIndex "
                                 "takes one header class")
        self.setup = DecodeSetup(h0)
        self.decoder = Decoder(self.setup, 1, max_batch, halfrate=halfrate)
        self.channels, self.rate, self.halfrate = self.setup.channels, self.decoder.rate, self.decoder.halfrate
        self.setups, self.file_class = [self.setup], np.zeros(len(headers), np.int32)
        self.file_channels = np.full(len(headers), self.channels, dtype=np.int64)
        self.file_rates = np.full(len(headers), self.rate)
        self.headers = [[bytes(p) for p in h] for h in headers]     # per file; the comment packets are the files' own
        self._hdr_pages, self._cutter = {}, None

    def decode_ranges(self, file_ids, starts, lengths):
        ln = np.asarray(lengths, dtype=np.int64)
        L = max(1, int(ln.max(initial=0)))
        dev = torch.device("cuda", torch.cuda.current_device())
        pcm = torch.zeros((len(ln), self.channels, L), dtype=torch.float32, device=dev)
        return self.decoder.synthesis_ranges(self.store, file_ids, starts, lengths, out=pcm)

    def _header_pages(self, f):
        """the pages that open a cut of file f (the cutter writes the cut's serial number into them): the class's
        identification and setup packets, the file's own comment packet"""
        from .stream import header_pages
        f = int(f)
        if f not in self._hdr_pages:
            self._hdr_pages[f] = header_pages(self.headers[f], 0)
        return self._hdr_pages[f]

    def _cutter_for(self, n, out_bytes, hdr_bytes):
        """the index's own cutter, grown (never shrunk) to hold such a call"""
        from .stream import OggCutter
        c = self._cutter
        if c is None or c.max_ranges < n or c.max_out_bytes < out_bytes or c.max_header_bytes < hdr_bytes:
            caps = (n, out_bytes, hdr_bytes) if c is None else (max(n, c.max_ranges), max(out_bytes, c.max_out_bytes),
                                                                max(hdr_bytes, c.max_header_bytes))
            if c is not None:
                c.close()
            self._cutter = c = OggCutter(max(1, caps[0]), caps[1], caps[2])
        return c

    def cut_ranges(self, file_ids, starts, lengths, serialnos=None, out=None, cutter=None):
        """Sample windows of the files as new .ogg files, the packets copied as they are (stream.OggCutter, rule:
        csrc/ogg_cut.h): file r decodes to decode_ranges' samples of (file_ids[r], starts[r], lengths[r]) with the
        source file's comments, under serial number serialnos[r] (None: r).  A window inside one packet starts at that
        packet's first sample; the starts and lengths returned say what every file holds.  A window past the file's
        end is an empty output, status 0; a window the packets cannot give is refused: empty, length 0, status
        stream.CUT_ESHAPE.
        -> ([bytes], starts int64 [n], lengths int64 [n], status int32 [n]): one call for the sizes, one that writes,
        and the outputs brought back in one copy.
        out=uint8 CUDA tensor: the single-call form, which only enqueues: -> (out_offsets int64 [n + 1], starts,
        lengths, status int32 [n + 1]) as device tensors, file r in out[out_offsets[r]:out_offsets[r + 1]], status[n]
        stream.CUT_ECAP when out is too small (nothing is written then).  cutter: an OggCutter of the caller's for the
        out= form, e.g. one per CUDA stream; without one the index keeps its own and regrows it as calls need."""
        from .stream import CUT_ECAP, CUT_ESHAPE
        if self.halfrate:
            raise ValueError("cut_ranges needs a full-rate index: half-rate positions are not packet granule positions")
        ids = np.asarray(file_ids, dtype=np.int64)
        n = len(ids)
        if ((ids < 0) | (ids >= len(self.headers))).any():
            raise ValueError("file id out of range")
        sn = np.arange(n, dtype=np.int64) if serialnos is None else np.asarray(serialnos, dtype=np.int64)
        if len(sn) != n:
            raise ValueError("serialnos needs one entry per range")
        pages = [self._header_pages(f) for f in ids]
        hb = sum(len(self._hdr_pages[f]) for f in set(ids.tolist()))
        if out is not None:
            c = cutter if cutter is not None else self._cutter_for(n, out.numel(), hb)
            off, stat, got_s, got_l = c.cut(self.store, ids, starts, lengths, pages, sn, out=out)
            dev = out.device
            got_l = torch.as_tensor(got_l, device=dev)
            got_l = torch.where(stat[:n] == CUT_ESHAPE, torch.zeros_like(got_l), got_l)
            return off, torch.as_tensor(got_s, device=dev), got_l, stat
        c = self._cutter_for(n, 0, hb)
        off, stat, got_s, got_l = c.cut(self.store, ids, starts, lengths, pages, sn)
        total = int(off[n].item())                            # the sizes: one small D2H
        c = self._cutter_for(n, total, hb)
        buf = torch.empty(max(total, 1), dtype=torch.uint8, device=c.device)
        off, stat, got_s, got_l = c.cut(self.store, ids, starts, lengths, pages, sn, out=buf[:total] if total else None)
        meta = torch.cat([off.view(torch.uint8), stat.view(torch.uint8), buf[:total]]).cpu().numpy()
        off, stat = meta[:8 * (n + 1)].view(np.int64), meta[8 * (n + 1):12 * (n + 1)].view(np.int32)
        if stat[n] not in (0, CUT_ECAP) or (stat[n] and total):
            raise VbmError(f"vbm_ogg_cut_ranges: status word {stat[n]}")
        raw = meta[12 * (n + 1):].tobytes()
        got_l[stat[:n] == CUT_ESHAPE] = 0
        return [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])], got_s, got_l, stat[:n].copy()

    def close(self):
        if self._cutter is not None:
            self._cutter.close()
            self._cutter = None
        self.store.close()
        self.decoder.close()
        for ds in self.setups:
            ds.close()


def _demux_files(files, device_demux, chained, multiplexed=False, resync=False):
    """decode_ogg's demux -> (names, entries, file_links): entry i, a file or with chained or resync a link, is a
    stream.Entry (headers, data, offsets, granulepos, eos, gap) as demux_ogg's, offsets a numpy array and the rest where the demux left them
    (CUDA tensors or numpy arrays), gap None without resync; file f is entries file_links[f] .. file_links[f + 1] - 1"""
    from .stream import Entry, _read_files, demux_ogg_device, demux_ogg_resync, split_ogg_chain
    if device_demux:
        b = demux_ogg_device(files, chained=chained, multiplexed=multiplexed, resync=resync)
        _raise_failed(b, b.names)
        offsets, entries = b.offsets.cpu().numpy(), []
        for i in range(len(b)):
            a, n, at = int(b.packet_base[i]), int(b.packets[i]), int(b.payload_base[i])
            entries.append(Entry(b.headers[i], b.payload[at:at + int(b.payload_bytes[i])], offsets[a:a + n + 1] - at,
                                 b.granulepos[a:a + n], b.eos[a:a + n], b.gaps(i) if resync else None))
        return b.names, entries, b.file_links
    names, entries, file_links = [], [], [0]
    if resync:
        for name, blob in zip(*_read_files(files)):
            for k, link in enumerate(demux_ogg_resync(blob)[0]):
                names.append(f"{name} link {k}")
                entries.append(link)
            file_links.append(len(entries))
        return names, entries, file_links
    for name, blob in zip(*_read_files(files)):
        if multiplexed:
            blob = _select_host(name, blob)
        links = [(f"{name} link {k}", link) for k, link in enumerate(split_ogg_chain(blob))] if chained else [(name, blob)]
        for entry, link in links:
            names.append(entry)
            entries.append(_demux_host(entry, link))
        file_links.append(len(entries))
    return names, entries, file_links


def _calls(src, max_packets):
    """The synthesis_runs calls over one group's streams, src[s] an entry of _demux_files (offsets on the host, the rest
    on the device), each yielded as (ids, counts, data, offsets, granulepos, eos, gap): its runs and their CSR; gap is
    None when the streams have none"""
    pos = [0] * len(src)
    while True:
        live = [s for s in range(len(src)) if pos[s] < len(src[s].offsets) - 1]
        if not live:
            return
        share, budget = max(1, max_packets // len(live)), max_packets
        ids, counts = [], []
        for s in live:                                    # the row budget in equal shares over the unfinished streams
            c = min(len(src[s].offsets) - 1 - pos[s], share, budget)
            if c <= 0:
                break
            ids.append(s)
            counts.append(c)
            budget -= c
        datas, offs, gps, eoss, gaps, base = [], [np.zeros(1, np.int64)], [], [], [], 0
        for s, c in zip(ids, counts):
            e, o = src[s], src[s].offsets
            if e.gap is not None:
                gaps.append(e.gap[pos[s]:pos[s] + c])
            a, b = int(o[pos[s]]), int(o[pos[s] + c])
            datas.append(e.data[a:b])
            offs.append(o[pos[s] + 1:pos[s] + c + 1] - a + base)
            gps.append(e.granulepos[pos[s]:pos[s] + c])
            eoss.append(e.eos[pos[s]:pos[s] + c])
            base += b - a
            pos[s] += c
        yield ids, counts, torch.cat(datas), np.concatenate(offs), torch.cat(gps), torch.cat(eoss), \
            torch.cat(gaps) if gaps else None


def decode_ogg(files, max_packets=4096, halfrate=False, device_demux=False, chained=False, multiplexed=False,
               one_decoder=False, resync=False):
    """.ogg files (bytes or paths), one logical stream each -> [(pcm float32 [channels, n] contiguous on the current
    device, rate)], one per file.  Files whose identification and setup headers are byte-equal share one DecodeSetup
    and Decoder, one stream per file; their packets go through synthesis_runs in calls of at most max_packets rows.
    Packets that fail to decode are skipped (as the reference's decoder_example.c skips them).  halfrate=True: half as
    many samples per file, and the rate returned is the output rate, half the file's (ov_halfrate).  Waits for the
    device once, at the end, to place the outputs.  device_demux=True: the files are demuxed together on the device
    (stream.DeviceDemuxer) instead of one by one on the host; the packet bytes then never leave the device, the offsets,
    granule positions and eos flags are read back once to plan the calls, and the PCM is the same bit for bit.
    chained=True: the files may be chained (stream.split_ogg_chain, csrc/ogg_chain.h), and the result is one list per
    file of (pcm, rate), one per link in file order.  Every link decodes as the file it would be alone: its own
    headers, fresh overlap state, its own granule positions; links and files with byte-equal identification and setup
    headers share a decoder.  A link that is not one valid logical stream raises VbmError naming file and link.
    multiplexed=True: the files may carry other streams beside the Vorbis one (Theora, Skeleton, Kate ...); the first
    Vorbis stream of a file, or with chained of each of its links, is decoded and the rest is ignored, as the
    reference's vorbisfile.c does (csrc/ogg_select.h; on the device with device_demux, stream.select_vorbis_stream on the
    host without).  A file without a Vorbis stream raises VbmError saying so.
    one_decoder=True: the files and links of all header classes go through one MixedDecoder, its caps the largest
    channel count and block size among them, in calls planned over all of them together instead of group by group;
    the result is the same, tensor for tensor.
    resync=True: the files may be damaged, chained or both (stream.ResyncDemuxer with device_demux, demux_ogg_resync on
    the host without; csrc/ogg_resync.h).  The result is one list per file of (pcm, rate), one per link that completed
    its three headers, empty for a file that has none; nothing is VBM_EOGG.  The packets go through synthesis_runs with
    the demux's gap marks, so behind a hole the decoder loses count as the reference's does ("out of sequence").  Whole
    header packets that no DecodeSetup takes raise VbmError naming file and link, as without the flag.  Not built
    together with multiplexed=True (ValueError)."""
    if max_packets <= 0:
        raise ValueError("max_packets must be positive")
    if resync and multiplexed:
        raise ValueError("decode_ogg: resync=True with multiplexed=True is not built")
    dev = torch.device("cuda", torch.cuda.current_device())
    names, demuxed, file_links = _demux_files(files, device_demux, chained, multiplexed, resync)
    groups = {}
    for i, d in enumerate(demuxed):
        groups.setdefault((d.headers[0], d.headers[2]), []).append(i)
    for members in groups.values():                       # every setup is checked before any work is enqueued
        rc = DecodeSetup.status(demuxed[members[0]].headers)
        if rc:
            raise VbmError(f"{names[members[0]]}: unsupported or invalid Vorbis headers (code {rc}): "
                           f"{lib.vbm_last_error().decode()}")
    pieces = [[] for _ in demuxed]                        # per entry: (pcm [channels, stride] view, index into lens)
    lens, keep, rates, nlens = [], [], [0] * len(demuxed), 0
    setups = []                                           # one DecodeSetup per group, in the groups' order

    def jobs():
        """(decoder, the entries that are its streams 0, 1, ...); without one_decoder each group's setup and decoder
        are made when its turn comes"""
        if one_decoder and groups:                        # one job: every entry a stream of one mixed decoder
            setups.extend(DecodeSetup(demuxed[members[0]].headers) for members in groups.values())
            md = MixedDecoder(len(demuxed), max_packets, max_classes=len(setups), halfrate=halfrate,
                              max_channels=max(ds.channels for ds in setups),
                              max_blocksize=max(ds.blocksizes[1] for ds in setups))
            keep.append(md)
            for ds, members in zip(setups, groups.values()):
                c = md.add_class(ds)
                for a in range(0, len(members), max_packets):         # one bind call takes max_batch streams
                    md.bind(members[a:a + max_packets], [c] * len(members[a:a + max_packets]))
            yield md, list(range(len(demuxed)))
            return
        for members in groups.values():                   # one job per header group
            setups.append(DecodeSetup(demuxed[members[0]].headers))
            keep.append(Decoder(setups[-1], len(members), max_packets, halfrate=halfrate))
            yield keep[-1], members

    for dec, members in jobs():
        up = lambda x: torch.as_tensor(x, device=dev)     # host-demuxed arrays go up here; demuxed on the device: as is
        src = [d._replace(data=up(d.data), granulepos=up(d.granulepos), eos=up(d.eos),
                          gap=None if d.gap is None else up(d.gap)) for d in (demuxed[j] for j in members)]
        for ids, counts, data, offsets, gp, eo, ga in _calls(src, max_packets):
            pcm, run_samples, _, _ = dec.synthesis_runs(ids, counts, data, torch.from_numpy(offsets).to(dev),
                                                        granulepos=gp, eos=eo, gap=ga)
            chans = dec.channels_of(ids) if one_decoder else [dec.channels] * len(ids)
            for r, s in enumerate(ids):
                pieces[members[s]].append((pcm[r, :chans[r]], nlens + r))
            lens.append(run_samples)
            nlens += len(ids)
    for ds, members in zip(setups, groups.values()):
        for j in members:
            rates[j] = output_rate(ds.rate, bool(halfrate))
            if not pieces[j]:
                pieces[j].append((torch.zeros((ds.channels, 0), dtype=torch.float32, device=dev), None))
    n = torch.cat(lens).cpu().tolist() if lens else []   # the one wait for the device
    out = []
    for j in range(len(demuxed)):
        parts = [p if k is None else p[:, :n[k]] for p, k in pieces[j]]
        out.append((torch.cat(parts, dim=1).contiguous(), rates[j]))
    for x in keep + setups:
        x.close()
    if chained or resync:
        return [out[int(file_links[f]):int(file_links[f + 1])] for f in range(len(file_links) - 1)]
    return out
