"""Batch Ogg demux, host twin (vbm_host_ogg_demux_scan / _fill, DeviceDemuxer(host=True)): every file of a batch comes out
byte for byte as vbm_ogg_demux gives it alone, or VBM_EOGG exactly when vbm_ogg_demux says so; one CSR for the batch; no
read outside a file; capacities and argument checks.  Host only: runs without a GPU."""
import ctypes as C
import mmap

import numpy as np
import pytest

from tests import ogg_demux_batch as B
from tests.ogg_demux_batch import EINVAL, EOGG, ECAP


def _check_batch(blobs, info, totals, res):
    assert res.status == 0 and res.canaries_ok
    B.check_csr(info, totals, res)
    for f, blob in enumerate(blobs):
        assert B.same(B.file_view(info, res, f), B.single(blob)), f


def test_mixed_batch_equals_single_file_demux():
    """the five _streams files and all corruptions in one batch, good and bad interleaved; reversed; each alone"""
    names, blobs = zip(*B.mixed())
    want = [B.single(b) for b in blobs]
    assert sum(w is None for w in want) == 11 and sum(w is not None for w in want) == 5
    info, totals, res = B.run("host", blobs)
    _check_batch(blobs, info, totals, res)
    views = [B.file_view(info, res, f) for f in range(len(blobs))]
    rinfo, rtotals, rres = B.run("host", blobs[::-1])
    _check_batch(blobs[::-1], rinfo, rtotals, rres)
    assert (rtotals == totals).all()
    for f in range(len(blobs)):
        assert B.same(B.file_view(rinfo, rres, len(blobs) - 1 - f), views[f]), names[f]
        ainfo, atotals, ares = B.run("host", [blobs[f]])
        assert B.same(B.file_view(ainfo, ares, 0), views[f]), names[f]
        assert ainfo[0]["status"] == info[f]["status"] and ainfo[0]["pages"] == info[f]["pages"]
    # failed files contribute nothing: the batch of the good files alone has the same outputs
    good = [b for b, w in zip(blobs, want) if w is not None]
    ginfo, gtotals, gres = B.run("host", good)
    assert (gtotals == totals).all()
    for name in ("headers", "payload", "offsets", "granulepos", "eos"):
        assert np.array_equal(getattr(gres, name), getattr(res, name)), name


def test_info_fields():
    import vorbis_aotuv_lancer_amd as v
    from tests.ogg_pages import split_pages
    names, blobs = zip(*B.mixed())
    info, _, _ = B.run("host", blobs)
    for f, blob in enumerate(blobs):
        if info[f]["status"] == 0:
            assert info[f]["pages"] == len(split_pages(blob)), names[f]
            assert info[f]["serialno"] == int.from_bytes(blob[14:18], "little"), names[f]
            assert [len(h) for h in v.demux_ogg(blob)[0]] == info[f]["header_bytes"].tolist()


def test_directed_shapes():
    """zero length, headers alone, 255 segments on a page, a packet over three pages, multiples of 255, a setup header
    that shares its page with audio, a header packet over pages, an unterminated last packet"""
    from tests.ogg_pages import split_pages
    d = dict(B.directed())
    blobs = list(d.values())
    info, totals, res = B.run("host", blobs)
    _check_batch(blobs, info, totals, res)
    st = dict(zip(d, info["status"].tolist()))
    assert st["zero length"] == EOGG and st["truncated"] == EOGG
    assert all(v == 0 for k, v in st.items() if k not in ("zero length", "truncated")), st
    pk = dict(zip(d, info["packets"].tolist()))
    assert pk["headers alone"] == 0 and pk["packet over three pages"] == 242 and pk["unterminated packet at the end"] == 240
    # the fixtures are what they are named
    three = split_pages(d["packet over three pages"])
    assert [p[26] for p in three[-3:]] == [255, 255, 6] and three[-2][5] & 1 and three[-1][5] & 1
    shared = split_pages(d["setup header shares its page"])
    assert sum(x < 255 for x in shared[1][27:27 + shared[1][26]]) >= 3        # comment, setup, audio
    spans = split_pages(d["header packet spans pages"])
    assert len(spans) >= 3 and spans[1][26] == 255 and spans[2][5] & 1
    # headers alone, and no file at all
    for blobs in ([d["headers alone"]], [d["zero length"]], []):
        info, totals, res = B.run("host", blobs)
        _check_batch(blobs, info, totals, res)
        assert totals[0] == 0 and totals[1] == 0 and res.offsets.tolist() == [0]


@pytest.mark.parametrize("first", [0, 1, 2, 3])
def test_file_start_alignments(first):
    """every file at every alignment: the buffer starts `first` bytes in, and one to three bytes of padding lie between
    the files, each pad a file of its own that fails and adds nothing"""
    good = [b for _, b in B.directed()[1:7]] + [B.mixed()[1][1]]
    blobs, is_pad = [], []
    for k, b in enumerate(good):
        blobs += [b"\xee" * (1 + k % 3), b]
        is_pad += [True, False]
    info, totals, res = B.run("host", blobs, first=first)
    _check_batch(blobs, info, totals, res)
    assert [bool(s) for s in info["status"]] == is_pad
    ref_info, ref_totals, ref = B.run("host", good)
    assert (totals == ref_totals).all()
    for name in ("headers", "payload", "offsets", "granulepos", "eos"):
        assert np.array_equal(getattr(res, name), getattr(ref, name)), name


def test_every_prefix_as_one_batch_against_an_unreadable_page():
    """every prefix of the six-packet file, all in one batch of adjacent files whose last byte is the last readable one:
    a prefix is what read_ogg makes of it (it ends on a page boundary) or VBM_EOGG"""
    import vorbis_aotuv_lancer_amd as v
    blob, bounds = B.six_packet_file()
    n = len(blob) + 1
    sizes = np.arange(n, dtype=np.int64)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    total = int(offsets[-1])
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    ps = mmap.PAGESIZE
    cap = (total + ps - 1) // ps * ps
    m = mmap.mmap(-1, cap + ps)
    base = C.addressof(C.c_char.from_buffer(m))
    assert libc.mprotect(C.c_void_p(base + cap), C.c_size_t(ps), 0) == 0          # PROT_NONE
    b = B.Batch("host", n, total)
    try:
        at = base + cap - total
        src = np.frombuffer(blob, np.uint8)
        dst = np.ctypeslib.as_array((C.c_ubyte * total).from_address(at))
        for k in range(n):
            dst[offsets[k]:offsets[k + 1]] = src[:k]
        info, totals = b.scan(at, offsets)
        res = b.fill(totals)
        del dst
    finally:
        b.close()
        libc.mprotect(C.c_void_p(base + cap), C.c_size_t(ps), 3)
        m.close()
    assert res.status == 0 and res.canaries_ok
    B.check_csr(info, totals, res)
    good = 0
    for k in range(n):
        got = B.file_view(info, res, k)
        assert (got is None) == (B.single(blob[:k]) is None), k
        if k not in bounds:                      # ends inside a page, or has no page at all
            assert got is None, k
            continue
        try:
            h, pk, gp, eos = v.read_ogg(blob[:k])
        except ValueError:                       # the first page alone: fewer than three packets
            assert got is None, k
            continue
        good += 1
        assert got[0] == [len(x) for x in h] and got[1] == b"".join(h), k
        assert [got[2][got[3][i]:got[3][i + 1]] for i in range(len(pk))] == pk, k
        assert got[4].tolist() == gp and [bool(e) for e in got[5]] == eos, k
        assert B.same(got, B.single(blob[:k])), k
    assert good >= 2


@pytest.mark.parametrize("short", ["packets", "payload", "headers"])
def test_capacity_one_short_writes_nothing(short):
    """fill with one capacity a single element below the batch's total: no buffer is written, canaries included, and
    the status word says so; the same demuxer then fills buffers that fit"""
    blobs = [b for _, b in B.mixed()[:6]]
    data, offsets = B.pack(blobs)
    b = B.Batch("host", len(blobs), len(data))
    try:
        info, totals = b.scan(data, offsets)
        assert all(int(t) > 0 for t in totals)
        res = b.fill(totals, short=short)
        assert res.status == ECAP and not res.touched and res.canaries_ok
        res = b.fill(totals)
        assert res.status == 0 and res.touched and res.canaries_ok
        B.check_csr(info, totals, res)
    finally:
        b.close()


def test_einval_cases():
    from vorbis_aotuv_lancer_amd._lib import lib
    blobs = [b for _, b in B.mixed()[:4]]
    data, offsets = B.pack(blobs)
    n, ptr = len(blobs), data.ctypes.data
    info = np.zeros(n, B._info_dtype())
    totals = np.zeros(3, np.int64)
    h = C.c_void_p()
    assert lib.vbm_host_ogg_demuxer_create(C.byref(h), 0, 100) == EINVAL
    assert lib.vbm_host_ogg_demuxer_create(C.byref(h), 4, -1) == EINVAL
    assert lib.vbm_host_ogg_demuxer_create(None, 4, 100) == EINVAL
    assert lib.vbm_host_ogg_demuxer_create(C.byref(h), n, len(data)) == 0
    scan, fill = lib.vbm_host_ogg_demux_scan, lib.vbm_host_ogg_demux_fill
    op, ip, tp = offsets.ctypes.data, info.ctypes.data, totals.ctypes.data
    out = [np.zeros(1 << 20, np.uint8), np.zeros(1 << 20, np.uint8), np.zeros(1 << 12, np.int64), np.zeros(1 << 12, np.int64),
           np.zeros(1 << 12, np.uint8)]
    hp, pp, fp, gp, ep = (a.ctypes.data for a in out)
    try:
        assert fill(h, hp, 1 << 20, pp, 1 << 20, fp, gp, ep, (1 << 12) - 1) == EINVAL           # fill without a scan
        assert scan(None, n, ptr, op, ip, tp) == EINVAL
        assert scan(h, -1, ptr, op, ip, tp) == EINVAL
        assert scan(h, n, None, op, ip, tp) == EINVAL
        assert scan(h, n, ptr, None, ip, tp) == EINVAL
        assert scan(h, n, ptr, op, None, tp) == EINVAL
        assert scan(h, n, ptr, op, ip, None) == EINVAL
        five = np.concatenate([offsets, offsets[-1:]])
        assert scan(h, n + 1, ptr, five.ctypes.data, ip, tp) == EINVAL                          # nfiles > max_files
        down = offsets.copy()
        down[2] = down[1] - 1
        assert scan(h, n, ptr, down.ctypes.data, ip, tp) == EINVAL                              # decreasing offsets
        neg = offsets.copy()
        neg[0] = -1
        assert scan(h, n, ptr, neg.ctypes.data, ip, tp) == EINVAL
        far = offsets.copy()
        far[-1] += 1
        assert scan(h, n, ptr, far.ctypes.data, ip, tp) == EINVAL                               # spans more than max_bytes
        assert lib.vbm_ogg_demux_scan(h, n, ptr, op, ip, tp, None) == EINVAL                    # a host demuxer in a device call
        assert fill(h, hp, 1 << 20, pp, 1 << 20, fp, gp, ep, (1 << 12) - 1) == EINVAL           # still no scan
        assert not info["status"].any() and not totals.any()
        assert scan(h, n, ptr, op, ip, tp) == 0
        assert fill(None, hp, 1 << 20, pp, 1 << 20, fp, gp, ep, (1 << 12) - 1) == EINVAL
        assert fill(h, None, 1 << 20, pp, 1 << 20, fp, gp, ep, (1 << 12) - 1) == EINVAL
        assert fill(h, hp, 1 << 20, None, 1 << 20, fp, gp, ep, (1 << 12) - 1) == EINVAL
        assert fill(h, hp, 1 << 20, pp, 1 << 20, None, gp, ep, (1 << 12) - 1) == EINVAL
        assert fill(h, hp, 1 << 20, pp, 1 << 20, fp, None, ep, (1 << 12) - 1) == EINVAL
        assert fill(h, hp, 1 << 20, pp, 1 << 20, fp, gp, None, (1 << 12) - 1) == EINVAL
        assert fill(h, hp, -1, pp, 1 << 20, fp, gp, ep, (1 << 12) - 1) == EINVAL
        assert fill(h, hp, 1 << 20, pp, -1, fp, gp, ep, (1 << 12) - 1) == EINVAL
        assert fill(h, hp, 1 << 20, pp, 1 << 20, fp, gp, ep, -1) == EINVAL
        assert lib.vbm_ogg_demux_fill(h, hp, 1 << 20, pp, 1 << 20, fp, gp, ep, (1 << 12) - 1, None) == EINVAL
        assert lib.vbm_ogg_demux_status(h, None, None) == EINVAL
        assert not any(a.any() for a in out)
        assert totals[1] < (1 << 20) and totals[0] < (1 << 12) - 1
        assert fill(h, hp, 1 << 20, pp, 1 << 20, fp, gp, ep, (1 << 12) - 1) == 0
        st = C.c_int(-1)
        assert lib.vbm_ogg_demux_status(h, C.byref(st), None) == 0 and st.value == 0
    finally:
        lib.vbm_ogg_demuxer_destroy(h)


def test_demux_ogg_device_host_twin():
    """the Python surface: per file (status, headers), one CSR for the batch, runs(f) in synthesis_runs form"""
    import vorbis_aotuv_lancer_amd as v
    names, blobs = zip(*B.mixed()[:7])
    b = v.demux_ogg_device(list(blobs), host=True)
    assert len(b) == len(blobs) and b.names == [f"file {i}" for i in range(len(blobs))]
    for f, blob in enumerate(blobs):
        try:
            h, data, offs, gp, eos = v.demux_ogg(blob)
        except v.VbmError:
            assert b.status[f] == EOGG and b.headers[f] is None and b.packets[f] == 0
            continue
        assert b.status[f] == 0 and b.headers[f] == h
        o, g, e = b.runs(f)
        assert np.array_equal(o - o[0], offs) and np.array_equal(g, gp) and np.array_equal(e, eos)
        assert np.array_equal(b.payload[o[0]:o[-1]], data) and o[0] == b.payload_base[f]
    dm = v.DeviceDemuxer(2, 10, host=True)
    with pytest.raises(v.VbmError):
        dm.demux([blobs[1]])                     # above max_bytes
    dm.close()
