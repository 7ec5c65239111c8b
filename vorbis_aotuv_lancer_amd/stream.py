"""Stream wrapper: the three Vorbis header packets of a Setup and Ogg page framing —
vorbis_analysis_headerout (reference lib/info.c:636-717) and libogg's ogg_stream_packetin/_pageout
(page format: reference doc/framing.html) over the C ABI of include/vorbis_mi355x.h.  OggStream / write_ogg page one
stream on the host; OggMux pages every stream of an encoder at once on the device (vbm_ogg_mux_*)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import lib, check, VbmError
from ._twin import HOST, Layout, _TwinHandle, ptr, size


def header_packets(setup, comments=(), vendor=None):
    """-> [identification, comment, setup] packets (bytes) = packets 0..2 of a stream"""
    arr = (C.c_char_p * max(len(comments), 1))(*[c.encode() if isinstance(c, str) else c for c in comments])
    lens = (C.c_long * 3)()
    v = vendor.encode() if isinstance(vendor, str) else vendor
    check(lib.vbm_header_packets(setup._h, v, arr, len(comments), None, 0, lens), "vbm_header_packets")
    total = sum(lens)
    buf = (C.c_ubyte * total)()
    check(lib.vbm_header_packets(setup._h, v, arr, len(comments), buf, total, lens), "vbm_header_packets")
    raw = bytes(buf)
    return [raw[:lens[0]], raw[lens[0]:lens[0] + lens[1]], raw[lens[0] + lens[1]:]]


class OggStream:
    """One logical Ogg bitstream (ogg_stream_state)."""

    def __init__(self, serialno):
        self._h = C.c_void_p()
        check(lib.vbm_ogg_stream_create(C.byref(self._h), serialno), "vbm_ogg_stream_create")

    def packetin(self, packet, granulepos, eos=False):
        check(lib.vbm_ogg_stream_packetin(self._h, packet, len(packet), 1 if eos else 0, granulepos),
              "vbm_ogg_stream_packetin")

    def pageout(self, flush=False):
        """-> bytes of the next complete page, or None when none is due"""
        page, n = C.c_void_p(), C.c_long()
        rc = lib.vbm_ogg_stream_pageout(self._h, 1 if flush else 0, C.byref(page), C.byref(n))
        if rc < 0:
            check(rc, "vbm_ogg_stream_pageout")
        return C.string_at(page, n.value) if rc == 1 else None

    def pages(self, flush=False):
        out = []
        while True:
            p = self.pageout(flush)
            if p is None:
                return out
            out.append(p)

    def close(self):
        if self._h:
            lib.vbm_ogg_stream_destroy(self._h)
            self._h = C.c_void_p()


def write_ogg(setup, packets, infos, serialno=1, comments=()):
    """Headers + the audio packets of ONE stream (in order, with their (granulepos, eos)) -> .ogg bytes,
    paged as the reference application does (examples/encoder_example.c:139-157, 211-233)."""
    os_ = OggStream(serialno)
    out = []
    for i, h in enumerate(header_packets(setup, comments)):
        os_.packetin(h, 0)
    out += os_.pages(flush=True)                     # audio data starts on a fresh page
    for pkt, (granulepos, eos) in zip(packets, infos):
        os_.packetin(pkt, granulepos, eos)
        out += os_.pages()
    out += os_.pages(flush=True)
    os_.close()
    return b"".join(out)


class OggMux:
    """Ogg paging for `nstreams` streams at once (vbm_ogg_mux_*): the pages write_ogg makes, byte for byte, from the rows
    an encode call leaves on the device.  serialnos: one per stream (default: the stream index).

        mux = OggMux(setup, S, enc.max_packet_bytes)
        headers = mux.start()                                 # list[bytes]: the header pages of every stream
        out, offsets, status = mux.mux(*fe.encode_rounds_device(2)[:3])
        # stream s of this call: out[offsets[s]:offsets[s + 1]]; status[s] != 0: see VBM_MUX_* in the C header

    mux() needs a GPU; mux_host() is its CPU twin over numpy arrays, with a state of its own.  start() resets both."""

    OK, EROWS, EQUEUE, ESTATE, EPACKET = 0, 1, 2, 3, 4

    def __init__(self, setup, nstreams, max_packet_bytes, serialnos=None, comments=(), max_rows_per_stream=16,
                 queue_bytes=0, device=None):
        import torch
        self.setup, self.nstreams, self.max_packet_bytes = setup, nstreams, max_packet_bytes
        self.serialnos = np.arange(nstreams, dtype=np.int32) if serialnos is None else \
            np.ascontiguousarray(serialnos).astype(np.uint32).astype(np.int32)
        if len(self.serialnos) != nstreams:
            raise ValueError("one serial number per stream")
        self.comments = [c.encode() if isinstance(c, str) else c for c in comments]
        self._hh, self._h = C.c_void_p(), C.c_void_p()
        check(lib.vbm_host_ogg_mux_create(C.byref(self._hh), setup._h, nstreams, max_packet_bytes, max_rows_per_stream,
                                          queue_bytes), "vbm_host_ogg_mux_create")
        self.device = None
        if device is not None or torch.cuda.is_available():
            self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            with torch.cuda.device(self.device):
                check(lib.vbm_ogg_mux_create(C.byref(self._h), setup._h, nstreams, max_packet_bytes, max_rows_per_stream,
                                             queue_bytes), "vbm_ogg_mux_create")
        self._ring, self._ring_rows, self._ring_at = None, -1, 0

    def out_bound(self, nrows):
        """most bytes one call with nrows rows can emit (vbm_ogg_mux_out_bound)"""
        return int(lib.vbm_ogg_mux_out_bound(self._hh, int(nrows)))

    def start(self, stream_ids=None, serialnos=None):
        """A new stream starts in each listed slot (default: all), optionally with new serial numbers -> the header
        pages of each as bytes, in the order listed."""
        ids = np.arange(self.nstreams, dtype=np.int32) if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        if serialnos is not None:
            self.serialnos[ids] = np.ascontiguousarray(serialnos).astype(np.uint32).astype(np.int32)
        sn = np.ascontiguousarray(self.serialnos[ids])
        n = len(ids)
        arr = (C.c_char_p * max(len(self.comments), 1))(*self.comments)
        off = np.zeros(n + 1, np.int64)
        buf = None
        for h, st in ((self._hh, None),) + (((self._h, C.c_void_p(self._stream())),) if self._h else ()):
            check(lib.vbm_ogg_mux_start_streams(h, ids.ctypes.data, n, sn.ctypes.data, None, arr, len(self.comments), None, 0,
                                                off.ctypes.data, st), "vbm_ogg_mux_start_streams")
            buf = np.zeros(max(int(off[n]), 1), np.uint8)
            check(lib.vbm_ogg_mux_start_streams(h, ids.ctypes.data, n, sn.ctypes.data, None, arr, len(self.comments),
                                                buf.ctypes.data, len(buf), off.ctypes.data, st), "vbm_ogg_mux_start_streams")
        raw = buf.tobytes()
        return [raw[off[k]:off[k + 1]] for k in range(n)]

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def mux(self, info, packets, nbytes, flush=False):
        """Rows of one encode call -> (out uint8 [capacity] on the device, offsets int64 [nstreams + 1], status int32
        [nstreams + 1]), all device tensors complete on the current stream: stream s got out[offsets[s]:offsets[s+1]],
        offsets[nstreams] bytes in all.  info: the device tensor of FrontEnd.encode_rounds_device, or the host records
        of encode_round / encode_rounds, which are uploaded on the current stream.  packets uint8 [n, stride >=
        max_packet_bytes], nbytes int32 [n] on the device.  The outputs live in a ring of three sets sized by
        vbm_ogg_mux_out_bound: a result stays valid until the third call after it."""
        import torch
        if not self._h:
            raise VbmError("OggMux.mux needs a GPU (mux_host is the CPU twin)")
        n = int(nbytes.shape[0])
        if isinstance(info, torch.Tensor):
            dinfo = info
        else:
            rec = np.ascontiguousarray(info)
            dinfo = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(self.device)
        if dinfo.numel() < n * 40 or int(packets.shape[0]) < n:
            raise ValueError("info and packets need one entry per row of nbytes")
        if n and not (packets.is_cuda and packets.dtype == torch.uint8 and packets.stride(-1) == 1 and nbytes.is_cuda
                      and nbytes.dtype == torch.int32 and nbytes.is_contiguous() and dinfo.is_contiguous()):
            raise ValueError("packets: CUDA uint8 rows, nbytes: contiguous CUDA int32")
        if self._ring is None or self._ring_rows < n:
            if self._ring is not None:
                torch.cuda.synchronize(self.device)
            cap = self.out_bound(n)
            self._ring = [(torch.empty((cap,), dtype=torch.uint8, device=self.device),
                           torch.zeros((self.nstreams + 1,), dtype=torch.int64, device=self.device),
                           torch.zeros((self.nstreams + 1,), dtype=torch.int32, device=self.device)) for _ in range(3)]
            self._ring_rows, self._ring_at = n, 0
        out, offsets, status = self._ring[self._ring_at]
        self._ring_at = (self._ring_at + 1) % 3
        stride = int(packets.stride(0)) if n and packets.dim() == 2 else self.max_packet_bytes
        check(lib.vbm_ogg_mux_packets(self._h, ptr(packets, n), stride, ptr(nbytes, n), ptr(dinfo, n), n,
                                      1 if flush else 0, out.data_ptr(), out.numel(),
                                      offsets.data_ptr(), status.data_ptr(), C.c_void_p(self._stream())),
              "vbm_ogg_mux_packets")
        self._keep = (dinfo, packets, nbytes)
        return out, offsets, status

    def mux_host(self, info, packets, nbytes, flush=False):
        """The CPU twin (vbm_host_ogg_mux_packets) over numpy arrays: info records (PacketInfo fields), packets uint8
        [n, stride], nbytes int32 [n] -> (out uint8 [bytes], offsets int64 [nstreams + 1], status int32 [nstreams + 1])."""
        nb = np.ascontiguousarray(nbytes, dtype=np.int32)
        n = len(nb)
        rec = np.ascontiguousarray(info)
        pk = np.ascontiguousarray(packets, dtype=np.uint8)
        if rec.nbytes < n * 40 or (n and (pk.ndim != 2 or pk.shape[0] < n)):
            raise ValueError("info and packets need one entry per row of nbytes")
        out = np.empty(self.out_bound(n), np.uint8)
        offsets = np.zeros(self.nstreams + 1, np.int64)
        status = np.zeros(self.nstreams + 1, np.int32)
        check(lib.vbm_host_ogg_mux_packets(self._hh, ptr(pk, n), pk.shape[1] if n else self.max_packet_bytes, ptr(nb, n),
                                           ptr(rec, n), n, 1 if flush else 0, out.ctypes.data, len(out),
                                           offsets.ctypes.data, status.ctypes.data), "vbm_host_ogg_mux_packets")
        return out[:offsets[-1]], offsets, status

    def close(self):
        if self._h:
            import torch
            torch.cuda.synchronize(self.device)
            self._ring = None
            lib.vbm_ogg_mux_destroy(self._h)
            self._h = C.c_void_p()
        if self._hh:
            lib.vbm_ogg_mux_destroy(self._hh)
            self._hh = C.c_void_p()


def _crc_table():
    t = []
    for i in range(256):
        r = i << 24
        for _ in range(8):
            r = ((r << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if r & 0x80000000 else (r << 1) & 0xFFFFFFFF
        t.append(r)
    return t


_CRC = _crc_table()


def _page_crc(page):
    crc = 0
    for b in page:
        crc = ((crc << 8) & 0xFFFFFFFF) ^ _CRC[((crc >> 24) & 0xFF) ^ b]
    return crc


def read_ogg(data):
    """.ogg bytes of ONE logical Vorbis stream -> (headers [3 packets], packets, granulepos, eos), the inverse of
    write_ogg (host only).  Pages are checked for the capture pattern, version and CRC (doc/framing.html); packets
    are reassembled from the lacing values across pages.  As libogg's ogg_stream_packetout reports them, a packet
    carries its page's granule position only if it is the last packet that ends on that page (-1 otherwise), and
    the end-of-stream flag only if it is the last packet of the stream's last page."""
    import struct
    data = bytes(data)
    pos, serial = 0, None
    out, gps, eoss = [], [], []
    partial = b""
    expect_seq = 0
    while pos < len(data):
        if data[pos:pos + 4] != b"OggS":
            raise ValueError(f"no Ogg capture pattern at byte {pos}")
        if len(data) < pos + 27:
            raise ValueError("truncated page header")
        version, flags, granule, sno, seq, crc, nseg = struct.unpack_from("<BBqIIIB", data, pos + 4)
        if version != 0:
            raise ValueError(f"unsupported Ogg version {version}")
        lacing = data[pos + 27:pos + 27 + nseg]
        body_len = sum(lacing)
        end = pos + 27 + nseg + body_len
        if len(lacing) != nseg or end > len(data):
            raise ValueError("truncated page")
        page = bytearray(data[pos:end])
        page[22:26] = b"\0\0\0\0"
        if _page_crc(page) != crc:
            raise ValueError(f"CRC mismatch in page {seq}")
        if serial is None:
            serial = sno
        elif sno != serial:
            raise ValueError("more than one logical stream (chained or multiplexed streams are not supported)")
        if seq != expect_seq:
            raise ValueError(f"page {seq} out of sequence (expected {expect_seq})")
        expect_seq += 1
        if not (flags & 1) and partial:
            raise ValueError("a packet continues into a page that is not marked as a continuation")
        body = data[pos + 27 + nseg:end]
        bpos, ended = 0, []
        for lv in lacing:
            partial += body[bpos:bpos + lv]
            bpos += lv
            if lv < 255:
                ended.append(partial)
                partial = b""
        for i, p in enumerate(ended):
            last = i == len(ended) - 1
            out.append(p)
            gps.append(granule if last else -1)
            eoss.append(bool(flags & 4) and last)
        pos = end
    if len(out) < 3:
        raise ValueError("fewer than three header packets")
    return out[:3], out[3:], gps[3:], eoss[3:]


def _split3(h, sizes, at=0):
    """-> the three header packets, of those sizes, that lie in the bytes h from h[at] on"""
    a, b, c = (int(x) for x in sizes[:3])
    return [h[at:at + a], h[at + a:at + a + b], h[at + a + b:at + a + b + c]]


# one demuxed file or link, as demux_ogg returns it, with the gap marks of a resync demux (None from any other) behind
Entry = namedtuple("Entry", "headers data offsets granulepos eos gap")


class _OggTwin(_TwinHandle):
    """A vbm_[host_]ogg_<kind> object, and the two halves of a demux call that the batch demuxers and the feed share"""

    def __init__(self, kind, host, device, *args, create="create"):
        self._destroy = f"vbm_ogg_{kind}_destroy"
        self._create(f"ogg_{kind}_{create}", host, device, *args)

    def _scan_meta(self, layout, *calls, zero=False):
        """The scan half: one block of that layout where the object's buffers live, then every call (stem, args), args
        being made from the addresses of the block's arrays ({name: address, None for an empty array}), then the block
        brought back in one small copy -> {name: that array on the host}"""
        block = self.mem.new(layout.size, np.uint8, zero)
        at = layout.ptrs(block)
        for stem, args in calls:
            self._call(stem, *args(at))
        return layout.views(self.mem.host(block))

    def _fill_csr(self, stem, P, B, H=None, gap=False, status=None):
        """The fill half, with buffers of the sizes the scan returned: vbm_[host_]<stem>([headers, H,] payload, B, offsets,
        granulepos, eos, [gap,] P) -> (the header bytes, payload, offsets, granulepos, eos, gap); the first is None
        without H and the last without gap.  With H the header bytes come back in one copy, which waits for the fill, and
        then the status word vbm_<status> is read: it is 0 with buffers of these sizes."""
        hdr = None if H is None else self.mem.new(H, np.uint8)
        payload, offsets, gp, eos = self.mem.csr(P, B)
        marks = self.mem.new(P, np.uint8) if gap else None
        self._call(stem, *((ptr(hdr, H), H) if H is not None else ()), ptr(payload, B), B, ptr(offsets), ptr(gp, P),
                   ptr(eos, P), *((ptr(marks, P),) if gap else ()), P)
        if H is not None:
            hdr = self.mem.host(hdr).tobytes()            # waits for the fill: the input is free after it
            st = self._status(status)
            if st:
                raise VbmError(f"vbm_{stem}: status {st} with buffers of the sizes the scan returned")
        return hdr, payload, offsets, gp, eos, marks


def demux_ogg(data):
    """read_ogg in C (vbm_ogg_demux), with the packets in CSR form for Decoder.synthesis_runs: .ogg bytes of ONE
    logical Vorbis stream -> (headers [3 packets], data uint8 [bytes], offsets int64 [P+1], granulepos int64 [P],
    eos uint8 [P]) as numpy arrays; audio packet k is data[offsets[k]:offsets[k+1]].  The same pages are rejected
    (VbmError instead of ValueError)."""
    raw = bytes(data)
    buf = (C.c_ubyte * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
    sizes = (C.c_long * 5)()
    check(lib.vbm_ogg_demux(buf, len(raw), sizes, None, None, None, None, None), "vbm_ogg_demux")
    hdr = np.zeros(max(1, sizes[0] + sizes[1] + sizes[2]), np.uint8)
    body, offsets, gp, eos = HOST.csr(sizes[3], sizes[4])
    check(lib.vbm_ogg_demux(buf, len(raw), sizes, hdr.ctypes.data, ptr(body, len(body)),
                            offsets.ctypes.data, gp.ctypes.data, eos.ctypes.data), "vbm_ogg_demux")
    return _split3(hdr.tobytes(), sizes), body, offsets, gp, eos


FILE_INFO = np.dtype([("status", "<i4"), ("pages", "<i4"), ("serialno", "<u4"), ("header_bytes", "<i4", (3,)),
                      ("packets", "<i8"), ("payload_bytes", "<i8"), ("packet_base", "<i8"), ("payload_base", "<i8"),
                      ("header_base", "<i8")])       # vbm_ogg_file_info


def demux_meta(n):
    """what vbm_ogg_demux_scan returns for n files, in one block"""
    return Layout(totals=(np.int64, 3), info=(FILE_INFO, n))


def _read_files(files):
    """bytes or paths -> (names, [bytes])"""
    import os
    names, blobs = [], []
    for i, f in enumerate(files):
        names.append(os.fspath(f) if isinstance(f, (str, os.PathLike)) else f"file {i}")
        if isinstance(f, (str, os.PathLike)):
            with open(f, "rb") as fh:
                f = fh.read()
        blobs.append(bytes(f))
    return names, blobs


class DemuxBatch:
    """What DeviceDemuxer.demux returns.  Per file f: status[f] (0 or VBM_EOGG), headers[f] ([3 packets] as bytes, None
    for a failed file), names[f], and info[f] (FILE_INFO: vbm_ogg_file_info).  For the batch: payload uint8 [bytes],
    offsets int64 [P + 1], granulepos int64 [P], eos uint8 [P] — torch tensors on the device (numpy arrays with
    host=True) holding ONE CSR over the audio packets of all good files: packet k of file f is
    payload[offsets[packet_base[f] + k]:offsets[packet_base[f] + k + 1]], with packets[f] of them.  runs(f) is that
    file's slice in the form Decoder.synthesis_runs takes.  From demux_ogg_device(chained=True) the entries ("files"
    above) are the links of the files given, named "<file> link k": file_links int64 [given files + 1] counts them, and
    links(f) is the range of entries of given file f.  Otherwise every file is its own one entry.  From
    demux_ogg_device(multiplexed=True) select_info holds one SELECT_INFO record per given file (vbm_ogg_select_info);
    None otherwise.  From a ResyncDemuxer (demux_ogg_device(resync=True)) the entries are the links that completed their
    headers, a given file may have none, gap uint8 [P] lies beside eos (1: something was lost in front of that packet;
    gaps(f) is entry f's slice) and events holds one RESYNC_EVENTS record per given file; both None otherwise."""

    def __init__(self, names, info, headers, payload, offsets, granulepos, eos, file_links=None, gap=None, events=None):
        self.names, self.info, self.headers = names, info, headers
        self.select_info = None
        self.gap, self.events = gap, events
        self.file_links = np.arange(len(names) + 1, dtype=np.int64) if file_links is None else file_links
        self.payload, self.offsets, self.granulepos, self.eos = payload, offsets, granulepos, eos
        self.status = info["status"].tolist()
        self.packets, self.packet_base = info["packets"], info["packet_base"]
        self.payload_bytes, self.payload_base = info["payload_bytes"], info["payload_base"]

    def __len__(self):
        return len(self.status)

    def runs(self, f):
        """-> (offsets [packets[f] + 1] as they stand (they index the whole payload), granulepos, eos) of file f"""
        a, n = int(self.packet_base[f]), int(self.packets[f])
        return self.offsets[a:a + n + 1], self.granulepos[a:a + n], self.eos[a:a + n]

    def links(self, f):
        """-> the entries that are the links of given file f"""
        return range(int(self.file_links[f]), int(self.file_links[f + 1]))

    def gaps(self, f):
        """-> entry f's slice of gap, beside runs(f): the marks Decoder.synthesis_runs(gap=...) takes (a ResyncDemuxer's
        batch only)"""
        a, n = int(self.packet_base[f]), int(self.packets[f])
        return self.gap[a:a + n]


class DeviceDemuxer(_OggTwin):
    """vbm_ogg_demux for many whole .ogg files per call, on the device (vbm_ogg_demux_scan / _fill): up to max_files
    files of up to max_bytes bytes together per demux() call.

        dm = DeviceDemuxer(len(files), sum(map(len, files)))
        b = dm.demux(files)                       # one H2D of the files, scan, a small D2H, fill, one D2H of the headers
        pcm, n, _, _ = dec.synthesis_runs([0], [b.packets[0]], b.payload, *b.runs(0))

    host=True runs the CPU twin on numpy arrays (no GPU needed).  A failed file (status VBM_EOGG) adds nothing to the
    batch and raises nothing here."""

    EOGG = -1002

    def __init__(self, max_files, max_bytes, host=False, device=None):
        self.max_files, self.max_bytes = int(max_files), int(max_bytes)
        super().__init__("demuxer", host, device, self.max_files, self.max_bytes)

    def demux(self, files):
        names, blobs = _read_files(files)
        return self.demux_joined(names, *self.mem.join(blobs))

    def demux_joined(self, names, raw, off):
        """demux() of files that already lie in one buffer: raw uint8 (a tensor on the device; a numpy array with
        host=True), entry i in raw[off[i]:off[i + 1]], off int64 numpy [n + 1]"""
        off = np.ascontiguousarray(off, np.int64)
        n = len(off) - 1
        meta = self._scan_meta(demux_meta(n), ("ogg_demux_scan", lambda at: (
            n, ptr(raw, len(raw)), off.ctypes.data, at["info"], at["totals"])))
        P, B, H = (int(x) for x in meta["totals"])
        h, payload, offsets, gp, eos, _ = self._fill_csr("ogg_demux_fill", P, B, H, status="ogg_demux_status")
        info = meta["info"]
        headers = [None if fi["status"] else _split3(h, fi["header_bytes"], int(fi["header_base"])) for fi in info]
        return DemuxBatch(names, info, headers, payload, offsets, gp, eos)


class ChainSplitter(_OggTwin):
    """Where the links of chained .ogg files start, for up to max_files files of up to max_bytes bytes together per
    split() call, on the device (vbm_ogg_chain_split; the rule: csrc/ogg_chain.h).  host=True runs the CPU twin on numpy
    arrays (no GPU needed).  The split never fails: what does not parse stays with the last link found, for the demux
    to reject."""

    ECAP = 1

    def __init__(self, max_files, max_bytes, host=False, device=None):
        self.max_files, self.max_bytes = int(max_files), int(max_bytes)
        super().__init__("chain", host, device, self.max_files, self.max_bytes)

    def split(self, raw, off, link_cap=None):
        """raw uint8 (a tensor on the device; a numpy array with host=True), file f in raw[off[f]:off[f + 1]], off int64
        numpy [n + 1] -> (file_links int64 [n + 1], link_offsets int64 [total + 1]) on the host: file f has links
        file_links[f] .. file_links[f + 1] - 1, and link j is raw[link_offsets[j]:link_offsets[j + 1]].  link_cap: the
        links the first try has room for (default 2 n + 62); a batch with more takes a second try with the exact total.
        One small D2H per try."""
        off = np.ascontiguousarray(off, np.int64)
        n = len(off) - 1
        cap = 2 * n + 62 if link_cap is None else int(link_cap)
        for attempt in range(2):
            # file_links and link_offsets in one buffer: one small D2H
            out = self.mem.new(n + cap + 2, np.int64)
            self._call("ogg_chain_split", n, ptr(raw, len(raw)), off.ctypes.data, ptr(out), ptr(out) + 8 * (n + 1), cap)
            out = self.mem.host(out)
            st = self._status("ogg_chain_status")
            total = int(out[n])
            if st == 0:
                return out[:n + 1].copy(), out[n + 1:n + total + 2].copy()
            if st != self.ECAP or attempt:
                break
            cap = total
        raise VbmError(f"vbm_ogg_chain_split: status {st} with room for the {total} links it counted")


def split_ogg_chain(data):
    """.ogg bytes of one file -> [bytes], its links (csrc/ogg_chain.h): a page with the beginning-of-stream flag that is
    not the file's first starts a link, and a file without one is its own one link.  On the host; needs no GPU.  The
    split never fails: each link is judged when it is demuxed (demux_ogg)."""
    raw = bytes(data)
    with ChainSplitter(1, len(raw), host=True) as sp:
        _, lo = sp.split(np.frombuffer(raw, np.uint8), np.array([0, len(raw)], np.int64))
    return [raw[int(a):int(b)] for a, b in zip(lo[:-1], lo[1:])]


RESYNC_EVENTS = np.dtype([("links_started", "<i4"), ("links_bad", "<i4"), ("gaps", "<i8"), ("skipped_bytes", "<i8"),
                          ("ignored_pages", "<i8"), ("pages", "<i8")])       # vbm_ogg_resync_events


def resync_meta(n, cap):
    """what vbm_ogg_resync_scan returns for n files with room for cap entries, in one block"""
    return Layout(totals=(np.int64, 6), links=(np.int64, n + 1), events=(RESYNC_EVENTS, n), info=(FILE_INFO, cap))


class ResyncDemuxer(_OggTwin):
    """The tolerant demux of many whole .ogg files per call, damaged, chained or both, on the device
    (vbm_ogg_resync_scan / _fill; the rule: csrc/ogg_resync.h): what the resync feed delivers from each file pushed whole.

        rd = ResyncDemuxer(len(files), sum(map(len, files)))
        b = rd.demux(files)                       # entries: the links that completed their headers; b.links(f) of file f
        pcm, n, _, _ = dec.synthesis_runs([0], [b.packets[e]], b.payload, *b.runs(e), gap=b.gaps(e))

    host=True runs the CPU twin on numpy arrays (no GPU needed).  max_candidates: the capture patterns the workspace has
    room for (default max_bytes // 27 + 2 * max_files + 64); a batch with more makes the object anew with the exact
    count and tries again, as does one with more entries than the first try had room for (2 n + 62)."""

    ECAP = 1
    # the capture search of the device form (csrc/ogg_resync.hip), in bytes from the dword that holds the buffer's first
    # byte: a lane's windows, a wavefront's, a row of 256 lanes, a tile of four rows, and the tiles of a full grid
    LANE, WAVE, ROW, TILE, GRID = 16, 1024, 4096, 16384, 1024 * 16384

    def __init__(self, max_files, max_bytes, host=False, device=None, max_candidates=None):
        self.max_files, self.max_bytes = int(max_files), int(max_bytes)
        self.max_candidates = self.max_bytes // 27 + 2 * self.max_files + 64 if max_candidates is None else int(max_candidates)
        super().__init__("resync", host, device, self.max_files, self.max_bytes, self.max_candidates)

    def demux(self, files):
        names, blobs = _read_files(files)
        return self.demux_joined(names, *self.mem.join(blobs))

    def _scan(self, n, raw, off, cap):
        """one scan with room for cap entries -> (totals [6], file_links [n + 1], events [n], info [cap]) on the host"""
        meta = self._scan_meta(resync_meta(n, cap), ("ogg_resync_scan", lambda at: (
            n, ptr(raw, len(raw)), off.ctypes.data, at["events"], at["links"], at["info"], cap, at["totals"])), zero=True)
        return meta["totals"], meta["links"].copy(), meta["events"].copy(), meta["info"]

    def demux_joined(self, names, raw, off, entry_cap=None):
        """demux() of files that already lie in one buffer: raw uint8 (a tensor on the device; a numpy array with
        host=True), file i in raw[off[i]:off[i + 1]], off int64 numpy [n + 1].  entry_cap: the entries the first try has
        room for."""
        off = np.ascontiguousarray(off, np.int64)
        n = len(off) - 1
        cap = 2 * n + 62 if entry_cap is None else int(entry_cap)
        for attempt in range(3):
            totals, file_links, events, info = self._scan(n, raw, off, cap)
            if int(totals[5]) == 0:
                break
            if int(totals[5]) != self.ECAP or attempt == 2:
                raise VbmError(f"vbm_ogg_resync_scan: status {int(totals[5])} with room for the counts it returned")
            if int(totals[4]) > self.max_candidates:             # the workspace is sized at create: a new object
                self.close()
                self.__init__(self.max_files, self.max_bytes, self.host, self.device, int(totals[4]))
            else:
                cap = int(totals[0])
        E, P, B, H = (int(x) for x in totals[:4])
        info = info[:E].copy()
        h, payload, offsets, gp, eos, gap = self._fill_csr("ogg_resync_fill", P, B, H, gap=True, status="ogg_resync_status")
        entry_names = [f"{names[f]} link {k}" for f in range(n) for k in range(int(file_links[f + 1] - file_links[f]))]
        headers = [_split3(h, fi["header_bytes"], int(fi["header_base"])) for fi in info]
        return DemuxBatch(entry_names, info, headers, payload, offsets, gp, eos, file_links, gap, events)


def demux_ogg_resync(data):
    """.ogg bytes of one file, damaged, chained or both -> (links, events), on the host (needs no GPU): every link that
    completed its three headers as (headers [3 packets], data uint8 [bytes], offsets int64 [P + 1], granulepos int64 [P],
    eos uint8 [P], gap uint8 [P]), audio packet k of the link in data[offsets[k]:offsets[k + 1]], and the file's
    RESYNC_EVENTS record.  Never fails: a file with nothing to deliver gives no link."""
    raw = bytes(data)
    with ResyncDemuxer(1, len(raw), host=True) as rd:
        b = rd.demux([raw])
    links = []
    for e in b.links(0):
        offs, gp, eos = b.runs(e)
        a, z = int(offs[0]), int(offs[-1])
        links.append(Entry(b.headers[e], b.payload[a:z].copy(), offs - a, gp.copy(), eos.copy(), b.gaps(e).copy()))
    return links, b.events[0]


SELECT_INFO = np.dtype([("kept_bytes", "<i8"), ("kept_pages", "<i8"), ("foreign_pages", "<i8"), ("streams", "<i4"),
                        ("foreign_streams", "<i4"), ("first_serial", "<u4"), ("reserved", "<i4")])   # vbm_ogg_select_info


def select_meta(n):
    """what vbm_ogg_select returns for n files beside the bytes it keeps, in one block"""
    return Layout(out_off=(np.int64, n + 1), info=(SELECT_INFO, n))


class StreamSelector(_OggTwin):
    """The Vorbis stream of multiplexed .ogg files (Theora, Skeleton, Kate ... pages between the audio's), for up to
    max_files files of up to max_bytes bytes together per select() call, on the device (vbm_ogg_select; the rule:
    csrc/ogg_select.h): the pages of the first Vorbis stream of every group are copied, whole and in order, to a second
    buffer and the rest is dropped, so that what comes out is a plain Vorbis file (or a plain chain) for DeviceDemuxer
    and ChainSplitter.  host=True runs the CPU twin on numpy arrays (no GPU needed).  The selection never fails: a file
    without a Vorbis stream comes out empty (info["streams"] == 0), for the demux to reject."""

    CHUNK = 16384       # VBM_OGG_SELECT_CHUNK: the output bytes one block of the copy kernel writes

    def __init__(self, max_files, max_bytes, host=False, device=None):
        self.max_files, self.max_bytes = int(max_files), int(max_bytes)
        super().__init__("select", host, device, self.max_files, self.max_bytes)

    def select(self, raw, off):
        """raw uint8 (a tensor on the device; a numpy array with host=True), file f in raw[off[f]:off[f + 1]], off int64
        numpy [n + 1] -> (out_raw, out_off, info): out_raw uint8 where raw is, the kept bytes of file f in
        out_raw[out_off[f]:out_off[f + 1]]; out_off int64 [n + 1] and info (SELECT_INFO [n]) on the host, brought back
        in one small D2H.  raw is free once the work enqueued here is done (the device form only enqueues it)."""
        off = np.ascontiguousarray(off, np.int64)
        n = len(off) - 1
        cap = int(off[n] - off[0])                       # the input's size always suffices: the status stays 0
        out = self.mem.new(cap, np.uint8)
        meta = self._scan_meta(select_meta(n), ("ogg_select", lambda at: (
            n, ptr(raw, len(raw)), off.ctypes.data, ptr(out, cap), cap, at["out_off"], at["info"])))
        out_off = meta["out_off"].copy()
        return out[:int(out_off[n])], out_off, meta["info"].copy()


def select_vorbis_stream(data):
    """.ogg bytes of one file -> bytes: the pages of its Vorbis stream alone (csrc/ogg_select.h), the first one of every
    group of a chained file; a plain Vorbis file comes back as it is, and a file without a Vorbis stream as b"".  On the
    host; needs no GPU.  The selection never fails: what it returns is judged when it is demuxed (demux_ogg)."""
    raw = bytes(data)
    with StreamSelector(1, len(raw), host=True) as sel:
        out, _, _ = sel.select(np.frombuffer(raw, np.uint8), np.array([0, len(raw)], np.int64))
    return out.tobytes()


def demux_ogg_device(files, host=False, chained=False, multiplexed=False, resync=False):
    """.ogg files (bytes or paths) -> DemuxBatch, through a DeviceDemuxer made for them (host=True: its CPU twin).
    chained=True: the files may be chained.  After the one upload a ChainSplitter finds their links, one small D2H brings
    the link offsets back, and the demuxer runs over the same buffer with the links as its files: the batch's entries
    are the links, b.links(f) those of file f, each judged alone (a bad link fails alone).
    multiplexed=True: the files may carry other streams beside the Vorbis one.  After the upload a StreamSelector copies
    the Vorbis pages of every file to a second device buffer, one small D2H brings the new file offsets and the records
    b.select_info (SELECT_INFO, one per given file) back, and the split and the demux run over that buffer.  A file
    without a Vorbis stream is an empty entry, which fails as one (VBM_EOGG).
    resync=True: the files may be damaged, chained or both, and come out through a ResyncDemuxer made for them: the
    entries are the links that completed their headers (chained is implied), none of them fails, and the batch has gap
    marks and events.  Not built together with multiplexed=True (ValueError)."""
    if resync and multiplexed:
        raise ValueError("demux_ogg_device: resync=True with multiplexed=True is not built")
    names, blobs = _read_files(files)
    nfiles, nbytes = max(1, len(blobs)), sum(len(b) for b in blobs)
    if resync:
        with ResyncDemuxer(nfiles, nbytes, host=host) as rd:
            return rd.demux_joined(names, *rd.mem.join(blobs))
    if not chained and not multiplexed:
        with DeviceDemuxer(nfiles, nbytes, host=host) as dm:
            return dm.demux(blobs)
    device, select_info, file_links = None, None, None
    raw = None
    if multiplexed:
        with StreamSelector(nfiles, nbytes, host=host) as sel:
            device = sel.device
            raw, off = sel.mem.join(blobs)
            raw, off, select_info = sel.select(raw, off)     # the D2H waits for the copy: the upload is free after it
    entry_names, entry_off = names, None if raw is None else off
    if chained:
        with ChainSplitter(nfiles, nbytes, host=host, device=device) as sp:
            device = sp.device
            if raw is None:
                raw, off = sp.mem.join(blobs)
            file_links, entry_off = sp.split(raw, off)
        entry_names = [f"{names[f]} link {k}" for f in range(len(blobs)) for k in range(int(file_links[f + 1] - file_links[f]))]
    with DeviceDemuxer(max(1, len(entry_names)), nbytes, host=host, device=device) as dm:
        b = dm.demux_joined(entry_names, raw, entry_off)
    if chained:
        b.file_links = file_links
    b.select_info = select_info
    return b


FEED_INFO = np.dtype([("status", "<i4"), ("headers_ready", "<i4"), ("header_bytes", "<i4", (3,)), ("serialno", "<u4"),
                      ("packets", "<i8"), ("payload_bytes", "<i8"), ("packet_base", "<i8"), ("payload_base", "<i8"),
                      ("pending", "<i8"), ("consumed", "<i8")])       # vbm_ogg_feed_info


FEED_EVENTS = np.dtype([("link", "<i4"), ("link_started", "<i4"), ("link_bad", "<i4"), ("gaps", "<i4"),
                        ("skipped_bytes", "<i8"), ("ignored_pages", "<i8"), ("left", "<i8")])    # vbm_ogg_feed_events


def feed_meta(n, resync):
    """what vbm_ogg_feed_scan, and from a resync feed vbm_ogg_feed_scan_events, return for n slots, in one block"""
    return Layout(totals=(np.int64, 2), info=(FEED_INFO, n), events=(FEED_EVENTS, n if resync else 0))


class FeedResult:
    """What OggFeed.push returns.  Per list entry i, on the host: ids[i], counts[i] (audio packets the call completed
    for that slot), status[i] (0, VBM_EOGG or VBM_OGG_FEED_EBIG: sticky) and info[i] (FEED_INFO: vbm_ogg_feed_info).
    For the call: payload uint8 [bytes], offsets int64 [P + 1], granulepos int64 [P], eos uint8 [P] — torch tensors on
    the device (numpy arrays with host=True) holding ONE CSR over the packets of all entries in list order.
    From a resync feed also: gap uint8 [P] beside eos (1: something was lost in front of that packet), and per list entry
    on the host events[i] (FEED_EVENTS: vbm_ogg_feed_events) with its fields left, link and link_started as arrays;
    None from a strict feed."""

    def __init__(self, ids, info, payload, offsets, granulepos, eos, gap=None, events=None):
        self.ids, self.info = ids, info
        self.payload, self.offsets, self.granulepos, self.eos = payload, offsets, granulepos, eos
        self.counts = info["packets"].astype(np.int64)
        self.status = info["status"].tolist()
        self.gap, self.events = gap, events
        self.left = self.link = self.link_started = None
        if events is not None:
            self.left = events["left"].astype(np.int64)
            self.link, self.link_started = events["link"].copy(), events["link_started"].astype(bool)

    def __len__(self):
        return len(self.ids)


class OggFeed(_OggTwin):
    """The Ogg demux for live streams (vbm_ogg_feed_scan / _fill): max_streams slots, each fed the next bytes of its
    stream, cut anywhere, up to max_call_bytes bytes per push() over all slots.

        feed = OggFeed(nstreams, nstreams * 8192)
        r = feed.push(ids, chunks)                # one H2D of the chunks, scan, a small D2H, fill
        live = [i for i, c in enumerate(r.counts) if c]
        pcm, n, _, _ = dec.synthesis_runs(r.ids[live], r.counts[live], r.payload, r.offsets,
                                          granulepos=r.granulepos, eos=r.eos)

    (with every listed slot live, r.ids and r.counts go in as they are).  feed.headers(id) returns the stream's three
    header packets once info["headers_ready"] is set.  host=True runs the CPU twin on numpy arrays (no GPU needed).

    resync=True makes the tolerant feed of a live mount (include/vorbis_mi355x.h, "Resync mode"): it follows chained
    links, joins mid-stream and goes on after lost or damaged pages.  A slot delivers packets of one link per call, so
    a chunk may come back in part (r.left); push_all pushes those parts again:

        feed = OggFeed(nstreams, nstreams * 8192, resync=True)
        for r in feed.push_all(ids, chunks):
            for i in np.flatnonzero((r.info["headers_ready"] != 0) & (r.link != link_of[r.ids])):
                ...                               # a new link: DecodeSetup(feed.headers(r.ids[i])), dec.restart_streams
                link_of[r.ids[i]] = r.link[i]     # (r.link_started marks the call its first page came in)
            live = np.flatnonzero(r.counts)
            dec.synthesis_runs(r.ids[live], r.counts[live], r.payload, r.offsets, granulepos=r.granulepos, eos=r.eos,
                               gap=r.gap)

    multiplexed=True (with or without resync) is for mounts that carry video, a Skeleton track or text beside the audio
    (include/vorbis_mi355x.h, "Multiplexed mode"): per slot, the pages of every stream but the group's first Vorbis
    stream are stepped over as they arrive, and push, push_all, headers and reset are used as before.  A resync feed
    counts them in events["ignored_pages"].  max_page_carry has to cover the largest foreign page."""

    EOGG, EBIG = -1002, -1003
    RESYNC, MULTIPLEXED = 1, 4

    def __init__(self, max_streams, max_call_bytes, max_page_carry=65307, max_packet_bytes=65536, header_cap=16384,
                 host=False, device=None, resync=False, multiplexed=False):
        self.max_streams, self.max_call_bytes, self.resync = int(max_streams), int(max_call_bytes), bool(resync)
        self.multiplexed = bool(multiplexed)
        args = (self.max_streams, self.max_call_bytes, int(max_page_carry), int(max_packet_bytes), int(header_cap))
        flags = (self.RESYNC if resync else 0) | (self.MULTIPLEXED if multiplexed else 0)
        if flags:
            super().__init__("feed", host, device, *args, flags, create="create2")
        else:
            super().__init__("feed", host, device, *args)

    def push(self, ids, chunks, end=False, offsets=None):
        """ids: the slots, each at most once.  chunks: one bytes-like per slot (uploaded in one copy), or ONE uint8
        tensor on the device (a numpy array with host=True) with offsets int64 [n + 1] on the host, chunk i being
        chunks[offsets[i]:offsets[i + 1]].  end: True / False for all, or one flag per slot.  -> FeedResult"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32))
        n = len(ids)
        if offsets is None:
            blobs = [bytes(c) for c in chunks]
            if len(blobs) != n:
                raise ValueError("one chunk per id")
            raw, off = self.mem.join(blobs)
        else:
            raw, off = chunks, np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
            if len(off) != n + 1:
                raise ValueError("offsets must have len(ids) + 1 entries")
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(end, dtype=np.uint8), (n,)))
        scans = [("ogg_feed_scan", lambda at: (n, ids.ctypes.data, ptr(raw, size(raw)), off.ctypes.data, flags.ctypes.data,
                                               at["info"], at["totals"]))]
        if self.resync:
            scans.append(("ogg_feed_scan_events", lambda at: (at["events"],)))
        with self.mem.scope():
            meta = self._scan_meta(feed_meta(n, self.resync), *scans)
            P, B = int(meta["totals"][0]), int(meta["totals"][1])
            # the buffers have the sizes the scan returned: this fill cannot fall short, so its status word is not waited for
            _, payload, offs, gp, eos, gap = self._fill_csr("ogg_feed_fill_gaps" if self.resync else "ogg_feed_fill", P, B,
                                                            gap=self.resync)
        return FeedResult(ids, meta["info"], payload, offs, gp, eos, gap, meta["events"] if self.resync else None)




    @staticmethod
    def _again(r, flags):
        """the entries to push again: bytes came back, or the end was given at a stop and carried bytes are still there"""
        if r.left is None:
            return []
        return np.flatnonzero((r.left > 0) | ((flags != 0) & (r.info["pending"] > 0)))

    def push_all(self, ids, chunks, end=False, offsets=None):
        """push() for a resync feed, again and again with the parts of the chunks that came back (r.left) until none is
        left; yields each FeedResult, whose ids are the slots that call listed.  `end` is passed on with every push (a
        slot honours it in the call that does not end at a stop; until then an entry is pushed again, with no bytes if
        none came back).  Chunks on the device are gathered with torch indexing."""
        ids = np.asarray(ids, dtype=np.int32)
        flags = np.broadcast_to(np.asarray(end, dtype=np.uint8), (len(ids),))
        if offsets is None:
            parts = [bytes(c) for c in chunks]
            if len(parts) != len(ids):
                raise ValueError("one chunk per id")
            while True:
                r = self.push(ids, parts, flags)
                yield r
                keep = self._again(r, flags)
                if len(keep) == 0:
                    return
                parts = [parts[i][len(parts[i]) - int(r.left[i]):] for i in keep]
                ids, flags = ids[keep], flags[keep]
        off = np.asarray(offsets, dtype=np.int64)
        while True:
            r = self.push(ids, chunks, flags, off)
            yield r
            keep = self._again(r, flags)
            if len(keep) == 0:
                return
            # the left parts, back to back
            a, b = off[1:][keep] - r.left[keep], off[1:][keep]
            noff = np.concatenate([[0], np.cumsum(b - a)]).astype(np.int64)
            idx = np.concatenate([np.arange(x, y) for x, y in zip(a, b)])
            chunks = chunks[self.mem.upload(idx)]           # indexing with an array gathers, on the host as on the device
            ids, flags, off = ids[keep], flags[keep], noff

    def headers(self, id):
        """-> the three header packets of slot `id` as bytes (for DecodeSetup); VbmError until they are complete"""
        sizes = (C.c_int * 3)()
        q = self._q()
        check(lib.vbm_ogg_feed_headers(self._h, int(id), None, 0, sizes, q), "vbm_ogg_feed_headers")
        buf = np.zeros(max(1, sum(sizes)), np.uint8)
        check(lib.vbm_ogg_feed_headers(self._h, int(id), buf.ctypes.data, sum(sizes), sizes, q), "vbm_ogg_feed_headers")
        return _split3(buf.tobytes(), sizes)

    def reset(self, ids):
        """those slots are free for new streams"""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32))
        check(lib.vbm_ogg_feed_reset_streams(self._h, len(ids), ids.ctypes.data, self._q()),
              "vbm_ogg_feed_reset_streams")


CUT_ECAP, CUT_ESHAPE = 1, 2      # VBM_OGG_CUT_ECAP (the call's status word), VBM_OGG_CUT_ESHAPE (a refused range)


def header_pages(headers, serialno):
    """The pages that open a stream with these three header packets under `serialno`, as write_ogg makes them -> bytes"""
    os_ = OggStream(serialno)
    try:
        for h in headers:
            os_.packetin(bytes(h), 0)
        return b"".join(os_.pages(flush=True))
    finally:
        os_.close()


class OggCutter(_OggTwin):
    """Sample windows of indexed streams as new Ogg Vorbis files with the packets left as they are (vbm_ogg_cut_*; the
    rule and the refusals: csrc/ogg_cut.h), for up to max_ranges windows, max_out_bytes output bytes and
    max_header_bytes of header pages per cut() call.  The device form cuts from a decoder.RangeStore and only enqueues
    on the current stream; one cutter serves one stream at a time (its workspace is the call's).  host=True runs the
    CPU twin over an index in numpy arrays (no GPU needed)."""

    def __init__(self, max_ranges, max_out_bytes, max_header_bytes, host=False, device=None):
        self.max_ranges, self.max_out_bytes = int(max_ranges), int(max_out_bytes)
        self.max_header_bytes = int(max_header_bytes)
        super().__init__("cut", host, device, self.max_ranges, self.max_out_bytes, self.max_header_bytes)

    def cut(self, src, stream_ids, starts, lengths, header_pages, serialnos=None, out=None):
        """src: a RangeStore (device form), or with host=True the index as a tuple of numpy arrays (first int64 [S + 1],
        status int32 [P], begin int32 [P], out_end int64 [P], totals int64 [S], data uint8, offsets int64 [P + 1]).
        header_pages: one bytes object per range, the pages that open its file (stream.header_pages, under any serial
        number: serialnos[r], or r without serialnos, is written into them); ranges that give the same bytes share
        one uploaded copy.  out: uint8 [cap], a tensor on the device (a numpy array with host=True), or None to ask for the
        sizes alone (the status word is then CUT_ECAP unless every output is empty).
        -> (out_offsets int64 [n + 1], status int32 [n + 1], got_starts int64 [n], got_lengths int64 [n]): the first
        two where out lives (device tensors that the enqueued work fills; numpy with host=True), the last two numpy.
        status[n] is the call's status word, status[r] 0 or CUT_ESHAPE; a refused range's length counts as 0."""
        ids = np.ascontiguousarray(stream_ids, np.int32)
        st, ln = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(lengths, np.int64)
        n = len(ids)
        if len(st) != n or len(ln) != n or len(header_pages) != n or (serialnos is not None and len(serialnos) != n):
            raise ValueError("stream_ids, starts, lengths, header_pages and serialnos need one entry per range")
        sn = None if serialnos is None else np.ascontiguousarray(np.asarray(serialnos, np.int64).astype(np.int32))
        sets, hid = {}, np.zeros(n, np.int32)
        for r, p in enumerate(header_pages):              # the distinct sets, in the order they first appear
            hid[r] = sets.setdefault(p, len(sets))
        hdr, hoff = HOST.join(list(sets))
        got_s, got_l = np.zeros(n, np.int64), np.zeros(n, np.int64)
        cap = 0 if out is None else int(size(out))
        off, stat = self.mem.new(n + 1, np.int64), self.mem.new(n + 1, np.int32)
        tail = (n, ids.ctypes.data, st.ctypes.data, ln.ctypes.data, ptr(sn), len(sets), ptr(hdr, len(hdr)), hoff.ctypes.data,
                hid.ctypes.data, ptr(out, cap), cap, ptr(off), ptr(stat), got_s.ctypes.data, got_l.ctypes.data)
        # the two forms differ in more than the stream here: the host twin takes the index as arrays, the device form a
        # store's handle (and its stream, which _call adds only behind a twin's own arguments)
        if self.host:
            first, status, begin, out_end, totals, data, offsets = src
            first, out_end, totals, offsets = (np.ascontiguousarray(a, np.int64) for a in (first, out_end, totals, offsets))
            status, begin = np.ascontiguousarray(status, np.int32), np.ascontiguousarray(begin, np.int32)
            data = np.ascontiguousarray(data, np.uint8)
            self._call("ogg_cut_ranges", len(first) - 1, first.ctypes.data, status.ctypes.data, begin.ctypes.data,
                       out_end.ctypes.data, totals.ctypes.data, ptr(data, len(data)), offsets.ctypes.data, len(data), *tail)
        else:
            self._call("ogg_cut_ranges", src._h, *tail, self._q())
        return off, stat, got_s, got_l
