"""Host Ogg demux in C (vbm_ogg_demux, demux_ogg): packet for packet what read_ogg returns, the same rejections, and no
read past the end of the data for any prefix of a valid file.  Host only: runs without a GPU."""
import ctypes as C
import mmap

import numpy as np
import pytest

from tests.ogg_demux_batch import streams
from tests.ogg_pages import corruptions, guarded_mapping, split_pages

EOGG = -1002


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
    for name, blob in streams(v):
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


def test_demux_rejects_what_read_ogg_rejects():
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    _, blob = streams(v)[1]
    for what, bad in corruptions(blob).items():
        with pytest.raises(ValueError):
            v.read_ogg(bad)
        buf = (C.c_ubyte * max(len(bad), 1)).from_buffer_copy(bad or b"\0")
        sizes = (C.c_long * 5)()
        rc = lib.vbm_ogg_demux(buf, len(bad), sizes, None, None, None, None, None)
        assert rc == EOGG, what
        with pytest.raises(v.VbmError):
            v.demux_ogg(bad)


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
    for p in split_pages(blob):
        pos += len(p)
        bounds.add(pos)
    m, base, cap = guarded_mapping(libc, len(blob))
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
    _, blob = streams(v)[0]
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
