"""Stream wrapper (host only): the three Vorbis header packets of a Setup and Ogg page framing —
vorbis_analysis_headerout (reference lib/info.c:636-717) and libogg's ogg_stream_packetin/_pageout
(page format: reference doc/framing.html) over the C ABI of include/vorbis_mi355x.h."""
import ctypes as C

import numpy as np

from ._lib import lib, check


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
    body = np.zeros(sizes[4], np.uint8)
    offsets = np.zeros(sizes[3] + 1, np.int64)
    gp = np.zeros(sizes[3], np.int64)
    eos = np.zeros(sizes[3], np.uint8)
    check(lib.vbm_ogg_demux(buf, len(raw), sizes, hdr.ctypes.data, body.ctypes.data if len(body) else None,
                            offsets.ctypes.data, gp.ctypes.data, eos.ctypes.data), "vbm_ogg_demux")
    h = hdr.tobytes()
    headers = [h[:sizes[0]], h[sizes[0]:sizes[0] + sizes[1]], h[sizes[0] + sizes[1]:sizes[0] + sizes[1] + sizes[2]]]
    return headers, body, offsets, gp, eos
