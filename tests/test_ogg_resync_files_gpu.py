"""The tolerant whole-file demux on the device (csrc/ogg_resync.hip: the byte-parallel capture search, one wavefront per
candidate, the resolve, the fill with gap marks): the inputs of the CPU file, every batch equal to the host twin in its
info and event structs, links, CSR, gap marks and headers, and equal to the byte-serial model."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ogg_feed_resync_cases as RC
from tests import ogg_resync_file_cases as F

pytestmark = pytest.mark.gpu


def both(blobs, first=0, **kw):
    blobs = [bytes(x) for x in blobs]
    dev, host = F.run("device", blobs, first, **kw), F.run("host", blobs, first, **kw)
    a, b = F.batch_bytes(dev), F.batch_bytes(host)
    assert a == b, [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert dev.payload.is_cuda and dev.gap.is_cuda and dev.gap.dtype == torch.uint8
    return F.check(dev, blobs)


def each_alone(blobs):
    rd = F.make("device", 1, max(len(x) for x in blobs))
    try:
        for x in blobs:
            F.check(F.run("device", [x], rd=rd), [x])
    finally:
        rd.close()


def test_the_interface_is_there(cuda):
    import vorbis_aotuv_lancer_amd as v
    b = v.demux_ogg_device([RC.paged_six(), b""], resync=True)
    assert b.gap.is_cuda and len(b) == 1 and list(b.links(1)) == [] and b.events["pages"].tolist()[1] == 0
    assert v.demux_ogg_device([RC.paged_six()], chained=True).gap is None


@pytest.mark.parametrize("first", (0, 1, 2, 3))
def test_undamaged_and_feed_damage(cuda, first):
    files, chains = F.undamaged()
    blobs = files + chains + list(F.feed_damage().values())
    b = both(blobs, first)
    assert not b.events["skipped_bytes"][:len(files) + len(chains)].any()
    if first == 0:
        each_alone(blobs)


@pytest.mark.parametrize("which", ("paged_six", "long_file"))
def test_removed_pages_and_flipped_bytes(cuda, which):
    blob = getattr(RC, which)()
    cases = F.removals(blob)
    b = both([c[0] for c in cases] + F.flips(blob), first=1)
    arrays = F.batch_arrays(b)
    for f, (_, want) in enumerate(cases):
        assert F.file_result(b, f, arrays)[0][0][1] == want, f
    if which == "paged_six":
        each_alone([c[0] for c in cases] + F.flips(blob))


def test_junk_at_every_page_boundary(cuda):
    blobs = F.junked(RC.paged_six())
    both(blobs)
    both(blobs, first=3)
    each_alone(blobs)
    both(F.junked(RC.long_file())[::7], first=2)


@pytest.mark.parametrize("first", (0, 1, 2, 3))
def test_the_smallest_inputs(cuda, first):
    blobs = F.tiny() + F.cut_headers() + F.edge_claims() + F.across_boundary() + F.shifted() + F.nested()
    both(blobs, first)
    for last in F.cut_headers()[:4] + F.tiny():          # ... each at the end of the whole buffer
        both([RC.paged_six(), last], first)
    if first == 0:
        each_alone(blobs)
        for x in F.shifted():                            # ... from the buffer's start
            both([x, RC.paged_six()])
    both([b""] * 5, first)
    both([], first)


def test_search_boundaries(cuda):
    """a capture pattern across every edge the search has below the grid's: dword, lane, wavefront, row, tile"""
    blobs = F.straddles()
    b = both(blobs)
    assert b.packets.tolist() == [6] * len(blobs) and not b.events["links_bad"].any()
    each_alone(blobs)
    both(blobs, first=1)


def test_search_grid_edge(cuda):
    """... and across the edge between the last tile of a full grid and the first tile of its next round"""
    import vorbis_aotuv_lancer_amd as v
    G = v.ResyncDemuxer.GRID
    size = G + 2 * v.ResyncDemuxer.TILE
    rd = F.make("device", 1, size)
    try:
        for d in (3, 2, 1, 0):
            blob = F.straddle_file(G - d, size)
            b = F.check(F.run("device", [blob], rd=rd), [blob])
            assert b.packets.tolist() == [6]
    finally:
        rd.close()


def test_65_files(cuda):
    both(F.sixty_five(), first=1)


def test_more_candidates_and_entries_than_there_is_room_for(cuda):
    blob, chain = F.many_candidates(), RC.chain_files()["3 links"]
    rd = F.make("device", 2, len(blob) + len(chain), max_candidates=10)
    raw, off = F.pack([blob, chain])
    d_raw = torch.from_numpy(raw.copy()).cuda()
    totals, links, events, info = rd._scan(2, d_raw, off, 8)
    want = (blob + chain).count(b"OggS")
    assert totals.tolist() == [0, 0, 0, 0, want, F.ECAP] and not links.any() and not info.view(np.uint8).any()
    b = F.check(rd.demux_joined(["f0", "f1"], d_raw, off, entry_cap=1), [blob, chain])     # two more tries
    assert rd.max_candidates == want and len(b) == 4
    totals, links, events, info = rd._scan(2, d_raw, off, 3)                           # one entry short
    assert totals[0] == 4 and totals[5] == F.ECAP and links.tolist() == [0, 1, 4] and not info.view(np.uint8).any()
    assert events.tobytes() == b.events.tobytes() and totals[1] == len(b.gap)
    rd.close()


def _fill(lib, rd, H, B, P, pad=8):
    """a device fill into buffers of these capacities with canaries behind them -> (status, [(bytes, capacity)])"""
    sizes = (H, B, (P + 1) * 8, P * 8, P, P)
    bufs = [torch.full((n + pad,), 0xA5, dtype=torch.uint8, device="cuda") for n in sizes]
    h, p, o, g, e, ga = (x.data_ptr() for x in bufs)
    assert lib.vbm_ogg_resync_fill(rd._h, h, H, p, B, o, g, e, ga, P, rd._q()) == 0
    st = C.c_int(-1)
    assert lib.vbm_ogg_resync_status(rd._h, C.byref(st), rd._q()) == 0
    return st.value, [(x.cpu().numpy(), n) for x, n in zip(bufs, sizes)]


def test_each_fill_capacity_one_short(cuda):
    import vorbis_aotuv_lancer_amd as v
    blobs = list(F.feed_damage().values())
    rd = F.make("device", len(blobs), sum(map(len, blobs)))
    raw, off = F.pack(blobs)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    totals, _, _, _ = rd._scan(len(blobs), d_raw, off, 64)
    E, P, B, H = (int(x) for x in totals[:4])
    for short in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        st, bufs = _fill(v.lib, rd, H - short[0], B - short[1], P - short[2])
        assert st == F.ECAP
        assert all((x == 0xA5).all() for x, _ in bufs), short          # nothing is written at all
    st, bufs = _fill(v.lib, rd, H, B, P)
    assert st == 0 and all((x[n:] == 0xA5).all() for x, n in bufs)
    b = F.run("host", blobs)
    for (x, n), y in zip(bufs[1:], F.batch_arrays(b)):
        assert x[:n].tobytes() == y.tobytes()
    rd.close()


def test_every_einval(cuda):
    """nothing is enqueued and nothing written"""
    import vorbis_aotuv_lancer_amd as v
    lib = v.lib
    blob = RC.paged_six()
    rd, host = F.make("device", 2, len(blob)), F.make("host", 2, len(blob))
    raw, off = F.pack([blob])
    d_raw = torch.from_numpy(raw.copy()).cuda()
    meta = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, q = meta.data_ptr(), rd._q()
    ok = dict(n=1, data=d_raw.data_ptr(), off=off.ctypes.data, ev=p + 512, links=p + 256, info=p + 1024, cap=4, tot=p)

    def scan(h=rd._h, **kw):
        a = dict(ok, **kw)
        return lib.vbm_ogg_resync_scan(h, a["n"], a["data"], a["off"], a["ev"], a["links"], a["info"], a["cap"], a["tot"], q)

    assert lib.vbm_ogg_resync_fill(rd._h, None, 0, None, 0, p, None, None, None, 0, q) == F.EINVAL          # no scan yet
    for kw in (dict(n=-1), dict(n=3), dict(off=None), dict(tot=None), dict(links=None), dict(ev=None), dict(info=None),
               dict(cap=-1), dict(data=None), dict(h=host._h), dict(h=None)):
        assert scan(**kw) == F.EINVAL, kw
    keep = [np.array(x, np.int64) for x in ((-1, 5), (5, 3), (0, len(blob) + 1))]
    for a in keep:
        assert scan(off=a.ctypes.data) == F.EINVAL, a
    assert lib.vbm_host_ogg_resync_scan(rd._h, 1, raw.ctypes.data, off.ctypes.data, None, None, None, 0, None) == F.EINVAL
    torch.cuda.synchronize()
    assert not meta.any()
    assert scan() == 0
    big = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    g = big.data_ptr()
    fill = lambda *a: lib.vbm_ogg_resync_fill(rd._h, *a, q)
    for a in ((g, -1, g, 0, g, g, g, g, 0), (g, 0, g, -1, g, g, g, g, 0), (g, 0, g, 0, g, g, g, g, -1),
              (g, 0, g, 0, None, g, g, g, 0), (None, 1, g, 0, g, g, g, g, 0), (g, 0, None, 1, g, g, g, g, 0),
              (g, 0, g, 0, g, None, g, g, 1), (g, 0, g, 0, g, g, None, g, 1), (g, 0, g, 0, g, g, g, None, 1)):
        assert fill(*a) == F.EINVAL, a
    assert lib.vbm_ogg_resync_fill(host._h, g, 0, g, 0, g, g, g, g, 0, q) == F.EINVAL
    torch.cuda.synchronize()
    assert not big.any()
    rd.close()
    host.close()


def test_two_demuxers_on_two_streams(cuda):
    """scan and fill of two demuxers enqueued on two streams with nothing waited for in between: each alone"""
    import vorbis_aotuv_lancer_amd as v
    lib = v.lib
    sets = [list(F.feed_damage().values()), F.junked(RC.paged_six())[:40]]
    want = [F.run("host", s) for s in sets]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rds, bufs = [], []
    for s in sets:
        rds.append(F.make("device", len(s), sum(map(len, s))))
    torch.cuda.synchronize()
    for rd, s, w, st in zip(rds, sets, want, streams):
        raw, off = F.pack(s)
        n, E, P = len(s), len(w), len(w.gap)
        B, H = len(w.payload), sum(len(x) for h in w.headers for x in h)
        with torch.cuda.stream(st):
            d_raw = torch.from_numpy(raw.copy()).cuda()
            meta = torch.zeros(48 + 8 * (n + 1) + 40 * n + 64 * E, dtype=torch.uint8, device="cuda")
            out = [torch.zeros(max(1, k), dtype=torch.uint8, device="cuda") for k in (H, B, 8 * (P + 1), 8 * P, P, P)]
            p, q = meta.data_ptr(), C.c_void_p(st.cuda_stream)
            assert lib.vbm_ogg_resync_scan(rd._h, n, d_raw.data_ptr(), off.ctypes.data, p + 48 + 8 * (n + 1), p + 48,
                                           p + 48 + 8 * (n + 1) + 40 * n, E, p, q) == 0
            assert lib.vbm_ogg_resync_fill(rd._h, *(x for o, c in zip(out[:2], (H, B)) for x in (o.data_ptr(), c)),
                                           *(o.data_ptr() for o in out[2:]), P, q) == 0
        bufs.append((d_raw, meta, out, (H, B, 8 * (P + 1), 8 * P, P, P)))
    torch.cuda.synchronize()
    for (d_raw, meta, out, sizes), w in zip(bufs, want):
        got = [o.cpu().numpy()[:k].tobytes() for o, k in zip(out, sizes)]
        assert got[0] == b"".join(x for h in w.headers for x in h)
        assert got[1:] == [x.tobytes() for x in F.batch_arrays(w)]
        n = len(w.file_links) - 1
        m = meta.cpu().numpy()
        assert m[48 + 8 * (n + 1):48 + 8 * (n + 1) + 40 * n].tobytes() == w.events.tobytes()
        assert m[48 + 8 * (n + 1) + 40 * n:].tobytes() == w.info.tobytes()
    for rd in rds:
        rd.close()
