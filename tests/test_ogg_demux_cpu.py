"""Host Ogg demux in C (vbm_ogg_demux, demux_ogg): packet for packet what read_ogg returns, the same rejections, and no
read past the end of the data for any prefix of a valid file.  Host only: runs without a GPU."""
import ctypes as C
import mmap
import struct

import numpy as np
import pytest

EOGG = -1002


def _streams(v):
    """(name, .ogg bytes) of write_ogg output: several classes' headers, with packets that span pages, packets whose
    lengths are multiples of 255 (0 included), and an eos packet"""
    rng = np.random.default_rng(5)
    out = []
    for ch, rate, q in [(1, 44100, 0.1), (2, 44100, 0.5), (6, 48000, 0.8), (2, 96000, 0.5)]:
        setup = v.Setup(ch, rate, q)
        lens = [1, 254, 255, 256, 510, 0, 765, 4097, 70000, 255 * 255, 255 * 255 + 1, 3, 255 * 3, 2, 300] * 2
        pk = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
        infos = [(-1 if k % 3 == 1 else 1024 * (k + 1), k == len(pk) - 1) for k in range(len(pk))]
        out.append((f"{ch}ch_{rate}_q{q}", v.write_ogg(setup, pk, infos, serialno=0x1234 + ch)))
    # many small packets: pages that close on the 4096-byte / 4-packet rule and on 255 segments
    setup = v.Setup(2, 44100, 0.5)
    pk = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 600, 700)]
    out.append(("small_packets", v.write_ogg(setup, pk, [(k * 512, k == len(pk) - 1) for k in range(len(pk))])))
    return out


def _same(v, blob):
    h, pk, gp, eos = v.read_ogg(blob)
    h2, data, offs, gp2, eos2 = v.demux_ogg(blob)
    assert h2 == h
    assert offs[0] == 0 and len(offs) == len(pk) + 1 and len(data) == offs[-1]
    assert [data[offs[k]:offs[k + 1]].tobytes() for k in range(len(pk))] == pk
    assert gp2.tolist() == gp
    assert [bool(e) for e in eos2] == eos


def test_demux_equals_read_ogg():
    import vorbis_aotuv_lancer_amd as v
    for name, blob in _streams(v):
        _same(v, blob)
        # page spans: at least one packet crosses a page
        assert blob.count(b"OggS") > 4, name


def test_demux_of_headers_alone():
    """a stream of the three header packets and no audio packet"""
    import vorbis_aotuv_lancer_amd as v
    blob = v.write_ogg(v.Setup(2, 44100, 0.5), [], [])
    h, data, offs, gp, eos = v.demux_ogg(blob)
    assert h == v.header_packets(v.Setup(2, 44100, 0.5))
    assert len(data) == 0 and offs.tolist() == [0] and len(gp) == 0 and len(eos) == 0


def _pages(blob):
    out, pos = [], 0
    while pos < len(blob):
        nseg = blob[pos + 26]
        end = pos + 27 + nseg + sum(blob[pos + 27:pos + 27 + nseg])
        out.append(bytearray(blob[pos:end]))
        pos = end
    return out


def _recrc(page):
    from vorbis_aotuv_lancer_amd.stream import _page_crc
    page[22:26] = b"\0\0\0\0"
    page[22:26] = struct.pack("<I", _page_crc(page))
    return page


def _corruptions(blob):
    pages = _pages(blob)
    j = b"".join
    cont = next(i for i, p in enumerate(pages) if p[5] & 1)            # a page that continues a packet
    out = {}
    bad = bytearray(blob)
    bad[0:4] = b"OggT"
    out["capture pattern"] = bytes(bad)
    out["capture pattern of page 2"] = j(pages[:2]) + b"Ogx" + j(pages[2:])[3:]
    p = [bytearray(x) for x in pages]
    p[1][4] = 1
    out["version"] = j(p[:1] + [_recrc(p[1])] + p[2:])
    bad = bytearray(blob)
    bad[len(pages[0]) + 40] ^= 0x10
    out["crc"] = bytes(bad)
    out["truncated page"] = blob[:-1]
    out["truncated header"] = j(pages) + pages[0][:20]
    p = [bytearray(x) for x in pages]
    p[2][14:18] = struct.pack("<I", 999)
    out["second serial"] = j(p[:2] + [_recrc(p[2])] + p[3:])
    out["out of sequence"] = j(pages[:2] + pages[3:])
    p = [bytearray(x) for x in pages]
    p[cont][5] &= ~1
    out["continuation without the flag"] = j(p[:cont] + [_recrc(p[cont])] + p[cont + 1:])
    out["fewer than three packets"] = j(pages[:1])
    out["empty"] = b""
    return out


def test_demux_rejects_what_read_ogg_rejects():
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    _, blob = _streams(v)[1]
    for what, bad in _corruptions(blob).items():
        with pytest.raises(ValueError):
            v.read_ogg(bad)
        buf = (C.c_ubyte * max(len(bad), 1)).from_buffer_copy(bad or b"\0")
        sizes = (C.c_long * 5)()
        rc = lib.vbm_ogg_demux(buf, len(bad), sizes, None, None, None, None, None)
        assert rc == EOGG, what
        with pytest.raises(v.VbmError):
            v.demux_ogg(bad)


def _guarded(libc, size):
    """an anonymous mapping whose page after `size` bytes (rounded up to pages) is inaccessible"""
    ps = mmap.PAGESIZE
    n = (size + ps - 1) // ps * ps
    m = mmap.mmap(-1, n + ps)
    base = C.addressof(C.c_char.from_buffer(m))
    assert libc.mprotect(C.c_void_p(base + n), C.c_size_t(ps), 0) == 0     # PROT_NONE
    return m, base, n


def test_demux_never_reads_past_n():
    """every prefix of a valid file, placed so that its last byte is the last readable byte: a prefix that ends on a
    page boundary demuxes as read_ogg does, any other is an error; none faults"""
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    setup = v.Setup(1, 44100, 0.1)
    rng = np.random.default_rng(9)
    pk = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (300, 255, 1, 600, 0, 2000)]
    blob = v.write_ogg(setup, pk, [(100 * k, k == len(pk) - 1) for k in range(len(pk))])
    bounds, pos = set(), 0
    for p in _pages(blob):
        pos += len(p)
        bounds.add(pos)
    m, base, cap = _guarded(libc, len(blob))
    sizes = (C.c_long * 5)()
    try:
        for n in range(len(blob) + 1):
            at = base + cap - n
            C.memmove(at, blob, n)
            rc = lib.vbm_ogg_demux(C.c_void_p(at), n, sizes, None, None, None, None, None)
            try:
                h, got, _, _ = v.read_ogg(blob[:n])
            except ValueError:
                assert rc == EOGG, n
                continue
            assert n in bounds and rc == 0, n
            assert list(sizes[:4]) == [len(x) for x in h] + [len(got)], n
    finally:
        libc.mprotect(C.c_void_p(base + cap), C.c_size_t(mmap.PAGESIZE), 3)
        m.close()
    _same(v, blob)


def test_demux_fill_call_checks_the_buffers():
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    _, blob = _streams(v)[0]
    buf = (C.c_ubyte * len(blob)).from_buffer_copy(blob)
    sizes = (C.c_long * 5)()
    assert lib.vbm_ogg_demux(buf, len(blob), sizes, None, None, None, None, None) == 0
    small = list(sizes)
    small[4] -= 1
    sizes2 = (C.c_long * 5)(*small)
    h = np.zeros(sum(small[:3]), np.uint8)
    d = np.zeros(small[4] + 1, np.uint8)
    o = np.zeros(small[3] + 1, np.int64)
    g = np.zeros(small[3], np.int64)
    e = np.zeros(small[3], np.uint8)
    assert lib.vbm_ogg_demux(buf, len(blob), sizes2, h.ctypes.data, d.ctypes.data, o.ctypes.data, g.ctypes.data,
                             e.ctypes.data) == -131
