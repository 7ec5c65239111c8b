"""Ogg cut on the MI355X (vbm_ogg_cut_ranges, OggIndex.cut_ranges): the device equals the host twin byte for byte
(outputs, offsets, status) on host-built and device-built stores; and the defining property, which no CPU check shows:
a cut decodes to exactly the samples that decode_ranges returns for the window.  The twin is pinned to the rule in
test_ogg_cut_cpu.py."""
import numpy as np
import pytest
import torch

from tests import ogg_cut_cases as K
from tests import ogg_select_cases as S
from tests.decode_packets import EINVAL
from tests.ogg_cut_cases import ECAP, ESHAPE
from tests.signals import synth_signal
from tests.ogg_pages import split_pages

pytestmark = pytest.mark.gpu

PADS = (300, 2000, 20000)         # the decoder and the store take packets of 20 000 bytes


def jitter_pad(packets, size):
    """K.pad to `size` and up to 15 bytes more, so that the packets start at every residue mod 16 in the store"""
    return [K.pad([p], size + (5 * j) % 16)[0] for j, p in enumerate(packets)]


@pytest.fixture(scope="module")
def world(cuda):
    """per header class the sources (files of 1.5 s from encode_ogg; for stereo also their packets padded, under another
    comment header), the windows over them, and what the twin makes of those"""
    import vorbis_aotuv_lancer_amd as v
    st = v.encode_ogg([synth_signal(2, 44100, 66150, seed=90 + i) for i in range(3)], 44100, quality=0.5,
                      serialnos=[51, 52, 53], comments=("title=source",))
    mono = v.encode_ogg([synth_signal(1, 44100, 66150, seed=95)], 44100, quality=0.5)[0]
    six = v.encode_ogg([synth_signal(6, 48000, 72000, seed=96)], 48000, quality=0.5)[0]
    two = [K.Source.from_blob(f"stereo {i}", b) for i, b in enumerate(st)]
    other = v.header_packets(v.Setup(2, 44100, 0.5), comments=("title=padded",))
    assert other[1] != two[0].headers[1] and other[0] == two[0].headers[0] and other[2] == two[0].headers[2]
    for i, size in enumerate(PADS):
        pk = two[i].packets()[:24 if size > 5000 else None]
        two.append(K.from_packets(f"padded {size}", other, jitter_pad(pk, size), "trim" if i == 1 else "plain"))
    classes = {"2ch": two, "1ch": [K.Source.from_blob("mono", mono)], "6ch": [K.Source.from_blob("six", six)]}
    w = {}
    for name, srcs in classes.items():
        ranges = []
        for i, src in enumerate(srcs):
            ranges += [(i, s, L, 1000 + 7 * len(ranges) + r) for r, (s, L) in enumerate(K.windows(src, 12, seed=20 + i))]
        store = K.Store(srcs)
        w[name] = dict(srcs=srcs, ranges=ranges, store=store, twin=K.run_twin(store, ranges))
    return w


def args(ranges):
    return tuple([r[c] for r in ranges] for c in range(4))


def open_index(v, srcs, device_demux, **kw):
    return v.OggIndex([s.blob for s in srcs], device_demux=device_demux, **kw)


@pytest.mark.parametrize("device_demux", [False, True])
@pytest.mark.parametrize("cls", ["2ch", "1ch", "6ch"])
def test_device_equals_twin(cuda, world, cls, device_demux):
    import vorbis_aotuv_lancer_amd as v
    w = world[cls]
    outs, off, stat, gs, gl, _ = w["twin"]
    n, total = len(w["ranges"]), int(off[-1])
    idx = open_index(v, w["srcs"], device_demux)
    try:
        assert np.array_equal(idx.total_samples, w["store"].totals)
        got, s, l, st = idx.cut_ranges(*args(w["ranges"]))                  # sizes, write, one copy back
        assert got == outs and np.array_equal(st, stat[:n]) and np.array_equal(s, gs) and np.array_equal(l, gl)
        assert (st == 0).sum() > n // 2 and any(o == b"" for o in outs)
        # the single call: exactly the total, a guard behind it
        buf = torch.full((total + 64,), 0xa5, dtype=torch.uint8, device=cuda)
        d_off, d_s, d_l, d_st = idx.cut_ranges(*args(w["ranges"]), out=buf[:total])
        assert all(t.is_cuda for t in (d_off, d_s, d_l, d_st))
        assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_st.cpu().numpy(), stat)
        assert np.array_equal(d_s.cpu().numpy(), gs) and np.array_equal(d_l.cpu().numpy(), gl)
        h = buf.cpu().numpy()
        assert h[:total].tobytes() == b"".join(outs) and (h[total:] == 0xa5).all()
        # one byte short: nothing written, offsets and status as they are
        buf.fill_(0xa5)
        d_off, _, _, d_st = idx.cut_ranges(*args(w["ranges"]), out=buf[:total - 1])
        assert np.array_equal(d_off.cpu().numpy(), off) and np.array_equal(d_st.cpu().numpy()[:n], stat[:n])
        assert int(d_st[n]) == ECAP and (buf.cpu().numpy() == 0xa5).all()
    finally:
        idx.close()


@pytest.mark.parametrize("cls", ["2ch", "1ch", "6ch"])
def test_a_cut_decodes_to_the_window(cuda, world, cls):
    """decode_ogg(cut r) == decode_ranges(file, start, length) of the returned start and length, sample for sample"""
    import vorbis_aotuv_lancer_amd as v
    w = world[cls]
    idx = open_index(v, w["srcs"], False)
    try:
        ids, starts, lengths, serials = args(w["ranges"])
        cuts, s, l, st = idx.cut_ranges(ids, starts, lengths, serials)
        keep = [r for r in range(len(cuts)) if cuts[r]]
        assert len(keep) > len(cuts) // 2 and all(st[r] == 0 and l[r] > 0 for r in keep)
        assert {ids[r] for r in keep} == set(range(len(w["srcs"])))        # every source, the padded ones too
        pcm, got = idx.decode_ranges([ids[r] for r in keep], s[keep], l[keep].astype(np.int32))
        assert np.array_equal(got, l[keep])
        dec = v.decode_ogg([cuts[r] for r in keep])
        want = pcm.cpu().numpy()
        for k, (r, (x, rate)) in enumerate(zip(keep, dec)):
            assert rate == idx.rate and x.shape == (idx.channels, int(l[r])), (r, w["ranges"][r])
            assert np.array_equal(x.cpu().numpy(), want[k, :, :int(l[r])]), (r, w["ranges"][r])
    finally:
        idx.close()


def test_padded_packets_start_at_every_residue(world):
    """the copy's alignment paths: source bytes at every offset mod 16, page bodies written at every offset mod 16"""
    w = world["2ch"]
    store, first = w["store"], w["store"].first
    for i in range(3, 3 + len(PADS)):
        assert {int(o) % 16 for o in store.offsets[first[i]:first[i + 1]]} == set(range(16)), w["srcs"][i].name
    outs, off = w["twin"][0], w["twin"][1]
    dst = set()
    for o, base in zip(outs, off):
        at = int(base)
        for p in split_pages(o):
            dst.add((at + 27 + p[26]) % 16)
            at += len(p)
    assert dst == set(range(16))


def test_two_cutters_on_two_streams_then_the_device_demux(cuda, world):
    """three calls each on two streams with no host wait between them; then the outputs are demuxed where they lie"""
    import vorbis_aotuv_lancer_amd as v
    w = world["2ch"]
    outs, off, stat = w["twin"][:3]
    good = [r for r in range(len(outs)) if outs[r]]
    calls = [[good[(3 * q + c)::6] for c in range(3)] for q in range(2)]      # six disjoint sets of non-empty cuts
    idx = open_index(v, w["srcs"], True)
    cap = max(sum(len(outs[r]) for r in rs) for q in calls for rs in q)
    hb = 6000 * max(len(rs) for q in calls for rs in q)
    cutters = [v.OggCutter(len(good), cap, hb) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    bufs = [[torch.zeros(cap, dtype=torch.uint8, device=cuda) for _ in range(3)] for _ in range(2)]
    res = [[None] * 3 for _ in range(2)]
    try:
        torch.cuda.synchronize()
        for c in range(3):
            for q in range(2):
                with torch.cuda.stream(streams[q]):
                    res[q][c] = idx.cut_ranges(*args([w["ranges"][r] for r in calls[q][c]]), out=bufs[q][c], cutter=cutters[q])
        torch.cuda.synchronize()
        for q in range(2):
            for c in range(3):
                want = [outs[r] for r in calls[q][c]]
                d_off = res[q][c][0].cpu().numpy()
                assert np.array_equal(np.diff(d_off), [len(x) for x in want]) and int(res[q][c][3][-1]) == 0
                assert bufs[q][c][:int(d_off[-1])].cpu().numpy().tobytes() == b"".join(want)
        # the demux over the device buffer: the packets pre .. m of every cut, from the device's own bytes
        rs, d_off = calls[0][0], res[0][0][0].cpu().numpy()
        dm = v.DeviceDemuxer(len(rs), cap)
        try:
            b = dm.demux_joined([f"cut {r}" for r in rs], bufs[0][0][:int(d_off[-1])], d_off)
        finally:
            dm.close()
        assert not any(b.status)
        payload, offsets = b.payload.cpu().numpy(), b.offsets.cpu().numpy()
        for f, r in enumerate(rs):
            i, s, L, _ = w["ranges"][r]
            src = w["srcs"][i]
            pre, k, m = K.model(src, s, L, 0)[4]
            a, n = int(b.packet_base[f]), int(b.packets[f])
            assert n == m - pre + 1 and b.headers[f] == src.headers
            assert payload[int(offsets[a]):int(offsets[a + n])].tobytes() == b"".join(src.packet(j) for j in range(pre, m + 1))
    finally:
        for c in cutters:
            c.close()
        idx.close()


def test_multiplexed_index_gives_the_same_cuts(cuda, world):
    import vorbis_aotuv_lancer_amd as v
    w = world["2ch"]
    src = w["srcs"][0]
    pages = [bytes(p) for p in split_pages(src.blob)]
    muxed = S._cat(S.interleave([S.foreign("theora", 72, 2, sizes=(150000, 30, 66000), max_segs=255), pages], 3))
    assert S.model(muxed)[0] == src.blob and muxed != src.blob
    wins = K.windows(src, 6, seed=31)
    a = v.OggIndex([muxed], device_demux=True, multiplexed=True)
    b = v.OggIndex([src.blob])
    try:
        call = ([0] * len(wins), [s for s, _ in wins], [L for _, L in wins])
        ga, gb = a.cut_ranges(*call), b.cut_ranges(*call)
        assert ga[0] == gb[0] and any(ga[0]) and all(np.array_equal(x, y) for x, y in zip(ga[1:], gb[1:]))
        assert ga[0] == [K.model(src, s, L, r)[0] for r, (s, L) in enumerate(wins)]
    finally:
        a.close()
        b.close()


def test_half_rate_is_refused(cuda, world):
    import vorbis_aotuv_lancer_amd as v
    src = world["2ch"]["srcs"][0]
    idx = v.OggIndex([src.blob], halfrate=True)
    c = v.OggCutter(1, 1 << 16, 1 << 14)
    try:
        with pytest.raises(ValueError, match="half-rate"):
            idx.cut_ranges([0], [0], [100])
        with pytest.raises(v.VbmError, match=str(EINVAL)):
            c.cut(idx.store, [0], [0], [100], [v.header_pages(src.headers, 0)])
    finally:
        c.close()
        idx.close()


def test_refusals_on_the_device(cuda):
    """the refusals of the CPU file, beside accepted ranges: the reference dumps under a lowered first granule, and
    packets of 40 000 bytes as pre and k"""
    import vorbis_aotuv_lancer_amd as v
    srcs = [K.dump_source("2ch-low"), K.dump_source("2ch-pad40000x8"), K.dump_source("2ch")]
    store = K.Store(srcs)
    low, big = srcs[0], srcs[1]
    j = int(np.flatnonzero(low.begin != 0)[0])
    ranges = [(2, 1000, 3000, 1), (0, int(low.out_start[j - 1]) + 1, int(low.out_end[j] - low.out_start[j - 1]) + 10, 2),
              (0, int(low.out_end[j]) + 5, 3000, 3), (0, int(low.out_start[j]) + 1, 5, 4), (1, int(big.out_start[3]) + 5, 2000, 5),
              (2, 5000, 100, 6)]
    outs, off, stat, gs, gl, _ = K.run_twin(store, ranges)
    assert list(stat[:-1]) == [0, ESHAPE, 0, ESHAPE, ESHAPE, 0]
    idx = open_index(v, srcs, False)
    try:
        got, s, l, st = idx.cut_ranges(*args(ranges))
        assert got == outs and np.array_equal(st, stat[:-1]) and np.array_equal(l, gl) and np.array_equal(s, gs)
    finally:
        idx.close()
