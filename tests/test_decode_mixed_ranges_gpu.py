"""Range stores, the device index, OggIndex and cut_ranges over several header classes.  The yardstick
is the single-class path: one Decoder + RangeStore + synthesis_ranges per class over the same windows of the same
streams (tests/decode_mixed_range_cases.py), itself pinned to the scalar inverse MDCT by the other decode suites.  Every
comparison is np.array_equal / torch.equal: there are no tolerances."""
import numpy as np
import pytest
import torch

from tests import decode_mixed_cases as M
from tests import decode_mixed_range_cases as R
from tests.decode_calls import runs_call
from tests.decode_packets import as_stream
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu

RATES = [False, True]
RATE_IDS = ["full", "half"]


def caps(classes):
    return dict(max_classes=len(classes), max_channels=max(k.ch for k in classes),
                max_blocksize=max(k.bs[1] for k in classes))


@pytest.fixture(scope="module")
def corpus(cuda):
    """the range streams, and per rate (made once, shared, never changed): their host index, the windows, the output
    stride and the yardstick's rows"""
    import vorbis_aotuv_lancer_amd as v
    classes, streams = R.range_streams()
    ds = [v.DecodeSetup(k.headers) for k in classes]
    cache = {}

    def at(halfrate):
        if halfrate not in cache:
            index = R.host_index(v, ds, streams, halfrate)
            windows = R.windows_of(index)
            stride = max(w[2] for w in windows)
            y = R.Yardstick(v, ds, streams, 4096, halfrate)
            want = y.ranges(windows, cuda, stride)
            y.close()
            cache[halfrate] = (index, windows, stride, want)
        return cache[halfrate]

    yield v, classes, ds, streams, at
    for d in ds:
        d.close()


def open_mixed(v, classes, ds, streams, cap, halfrate=False, nstreams=1):
    md = v.MixedDecoder(nstreams, cap, halfrate=halfrate, **caps(classes))
    cid = [md.add_class(d) for d in ds]
    store = v.RangeStore(md, [as_stream(pk) for _, pk in streams], classes=[cid[c] for c, _ in streams])
    return md, store


def run_mixed(v, classes, ds, streams, windows, stride, cap, dev, halfrate=False):
    md, store = open_mixed(v, classes, ds, streams, cap, halfrate)
    pcm, got = R.mixed_ranges(v, md, store, windows, dev, stride)
    pcm = pcm.cpu().numpy()
    store.close()
    md.close()
    return pcm, got


@pytest.mark.parametrize("halfrate", RATES, ids=RATE_IDS)
def test_colliding_classes_in_one_call(cuda, corpus, halfrate):
    """eight streams of five classes that share transform sizes, every kind of window of every stream, one store and
    one call; tests 1 and 3 of the issue"""
    v, classes, ds, streams, at = corpus
    index, windows, stride, want = at(halfrate)
    assert len(windows) == 8 * len(streams) and all(streams[a][0] != streams[a + 1][0] for a in range(len(streams) - 1))
    assert all(pk[-1][2] == 1 and pk[-1][1] >= 0 for _, pk in streams)          # a trimming granule position, e_o_s
    pcm, got = run_mixed(v, classes, ds, streams, windows, stride, 4096, cuda, halfrate)
    chans = [classes[streams[w[0]][0]].ch for w in windows]
    assert R.same_ranges(pcm, got, want, chans) > 0
    kinds = [[int(got[k * len(streams) + s]) for s in range(len(streams))] for k in range(8)]
    assert kinds[0] == [ix[4] for ix in index] and all(g == 10 for g in kinds[2]) and all(g == 50 for g in kinds[3])
    assert kinds[4] == [0] * len(streams) and kinds[5] == [0] * len(streams)


def test_pieces_and_sub_calls_of_several_classes(cuda, corpus):
    """max_batch = 5: windows split into pieces and sub-calls, some of which hold pieces of two classes"""
    v, classes, ds, streams, at = corpus
    index, windows, stride, _ = at(False)
    first = np.cumsum([0] + [len(pk) for _, pk in streams])
    status = np.concatenate([ix[0] for ix in index])
    out_end = np.concatenate([ix[3] + (ix[2] - ix[1]) for ix in index])
    calls = R.plan_calls(first, status, out_end, [ix[4] for ix in index], 5, windows)
    assert len(calls) > len(windows) // 2 and all(len(c) <= 2 for c in calls)    # at most two pieces in five rows
    assert any(len({streams[i][0] for i in c}) == 2 for c in calls), "no sub-call with pieces of two classes"
    assert any(len(set(c)) == 1 and len(c) == 1 for c in calls)
    small = run_mixed(v, classes, ds, streams, windows, stride, 5, cuda)
    large = run_mixed(v, classes, ds, streams, windows, stride, 4096, cuda)
    assert np.array_equal(small[1], large[1]) and np.array_equal(small[0], large[0])


@pytest.mark.parametrize("halfrate", RATES, ids=RATE_IDS)
def test_index_of_several_classes(cuda, halfrate):
    import vorbis_aotuv_lancer_amd as v
    classes, streams = R.index_streams()
    of = [c for c, _ in streams]
    assert len(set(of[:4])) == 4
    ds = [v.DecodeSetup(k.headers) for k in classes]
    md = v.MixedDecoder(1, 64, halfrate=halfrate, **caps(classes))
    cid = [md.add_class(d) for d in ds]
    data, offs, gp, eo, first = R.csr(streams)
    t = [torch.from_numpy(a).to(cuda) for a in (data, offs, gp, eo)]
    got = v.decode_index_device(md, *t, stream_packets=first, classes=[cid[c] for c in of])
    status, begin, end, out_start, totals = (x.cpu().numpy() for x in got)
    want = R.host_index(v, ds, streams, halfrate)
    for i, (st, b, e, o, total) in enumerate(want):
        a, z = int(first[i]), int(first[i + 1])
        assert np.array_equal(status[a:z], st) and np.array_equal(begin[a:z], b) and np.array_equal(end[a:z], e), i
        assert np.array_equal(out_start[a:z], o) and totals[i] == total, i
    host = v.RangeStore(md, [as_stream(pk) for _, pk in streams], classes=[cid[c] for c in of])
    dev = v.RangeStore.from_device(md, *t, stream_packets=first, classes=[cid[c] for c in of])
    assert np.array_equal(host.totals, totals) and np.array_equal(dev.totals, totals)
    windows = []
    for s, ix in enumerate(want):
        windows += [(s, 0, min(ix[4], 700)), (s, ix[4] // 3, 200)]
    a, ga = R.mixed_ranges(v, md, host, windows, cuda, 700)
    b, gb = R.mixed_ranges(v, md, dev, windows, cuda, 700)
    assert np.array_equal(ga, gb) and ga.sum() > 0 and torch.equal(a, b)
    assert ga[2 * 9] == 0 and ga[2 * 10] > 0                           # the empty stream, the one with failed packets
    for x in (host, dev, md, *ds):
        x.close()


def runs(md, parts, dev):
    return runs_call(md, [s for s, _ in parts], [r for _, r in parts], dev)[:2]


def test_range_calls_leave_bound_streams_alone(cuda, corpus):
    v, classes, ds, streams, at = corpus
    _, windows, stride, _ = at(False)
    md, store = open_mixed(v, classes, ds, streams, 4096, nstreams=2)
    pick = [0, 2]                                                      # mono (256, 512) and 3 channels (512, 4096)
    bound = {s: streams[j][1] for s, j in enumerate(pick)}
    md.bind([0, 1], [streams[j][0] for j in pick])
    a1 = runs(md, [(s, pk[:6]) for s, pk in bound.items()], cuda)
    _, got = R.mixed_ranges(v, md, store, windows, cuda, stride)
    a2 = runs(md, [(s, pk[6:]) for s, pk in bound.items()], cuda)
    md.bind([0, 1], [streams[j][0] for j in pick])                     # restarts: the uninterrupted decode
    b1 = runs(md, [(s, pk[:6]) for s, pk in bound.items()], cuda)
    b2 = runs(md, [(s, pk[6:]) for s, pk in bound.items()], cuda)
    assert got.sum() > 0
    for (pa, na), (pb, nb) in ((a1, b1), (a2, b2)):
        assert torch.equal(na, nb) and (na > 0).all()
        for r, n in enumerate(na.cpu().tolist()):
            ch = classes[streams[pick[r]][0]].ch
            assert torch.equal(pa[r, :ch, :n], pb[r, :ch, :n])
    store.close()
    md.close()


def test_class_added_after_the_first_store(cuda, corpus):
    v, classes, ds, streams, at = corpus
    _, windows, stride, want = at(False)
    md = v.MixedDecoder(1, 4096, **caps(classes))
    cid = [md.add_class(ds[0]), md.add_class(ds[1])]
    early = [s for s, (c, _) in enumerate(streams) if c < 2]
    store1 = v.RangeStore(md, [as_stream(streams[s][1]) for s in early], classes=[cid[streams[s][0]] for s in early])
    cid += [md.add_class(d) for d in ds[2:]]
    store2 = v.RangeStore(md, [as_stream(pk) for _, pk in streams], classes=[cid[c] for c, _ in streams])
    rows1 = [r for r, w in enumerate(windows) if w[0] in early]
    w1 = [(early.index(windows[r][0]),) + windows[r][1:] for r in rows1]
    chans = [classes[streams[w[0]][0]].ch for w in windows]
    out = [R.mixed_ranges(v, md, st, w, cuda, stride) for st, w in ((store1, w1), (store2, windows)) * 2]
    for k, (pcm, got) in enumerate(out):                               # the first wait for the device is here
        mine = rows1 if k % 2 == 0 else range(len(windows))
        assert R.same_ranges(pcm.cpu().numpy(), got, [want[r] for r in mine], [chans[r] for r in mine]) > 0
    for x in (store1, store2, md):
        x.close()


@pytest.fixture(scope="module")
def encoded(cuda):
    """five real files of two header classes (stereo 44100 q5, mono 8 kHz), each under 2 s, as
    tests/test_decode_mixed_gpu.py makes them"""
    import vorbis_aotuv_lancer_amd as v
    stereo = v.encode_ogg([synth_signal(2, 44100, n, seed=3 + i) for i, n in enumerate((40001, 30000, 4099))], 44100,
                          quality=0.5, serialnos=[11, 12, 13])
    mono = v.encode_ogg([synth_signal(1, 8000, n, seed=8 + i) for i, n in enumerate((15000, 2500))], 8000, quality=0.5,
                        serialnos=[21, 22])
    return [stereo[0], mono[0], stereo[1], stereo[2], mono[1]]


def seeded_windows(totals, n, seed):
    rng = np.random.default_rng(seed)
    f = np.concatenate([np.arange(len(totals)), rng.integers(0, len(totals), n - len(totals))])
    starts = np.array([rng.integers(0, totals[i]) for i in f], np.int64)
    return f, starts, rng.integers(1, 3000, n)


def check_windows(ix, want, f, starts, lengths):
    pcm, got = ix.decode_ranges(f, starts, lengths)
    assert tuple(pcm.shape) == (len(f), ix.channels, int(max(lengths)))
    for r in range(len(f)):
        full, ch, g = want[f[r]][0], int(ix.file_channels[f[r]]), int(got[r])
        assert g == min(int(lengths[r]), full.shape[1] - int(starts[r])) and g > 0
        assert torch.equal(pcm[r, :ch, :g], full[:, int(starts[r]):int(starts[r]) + g]), r
        assert not pcm[r, ch:].any() and not pcm[r, :, g:].any(), r
    return pcm, got


@pytest.mark.parametrize("kw", [dict(), dict(device_demux=True), dict(halfrate=True)], ids=["host", "device", "half"])
def test_ogg_index_one_decoder(cuda, encoded, kw):
    import vorbis_aotuv_lancer_amd as v
    half = bool(kw.get("halfrate"))
    want = v.decode_ogg(encoded, halfrate=half)
    ix = v.OggIndex(encoded, one_decoder=True, **kw)
    assert ix.total_samples.tolist() == [p.shape[1] for p, _ in want]
    assert ix.file_channels.tolist() == [2, 1, 2, 2, 1] and ix.channels == 2 and ix.rate is None
    assert ix.file_rates.tolist() == [r for _, r in want] and ix.file_rates[1] == (4000 if half else 8000)
    f, starts, lengths = seeded_windows(ix.total_samples, 20, 5)
    assert set(f.tolist()) == {0, 1, 2, 3, 4}
    check_windows(ix, want, f, starts, lengths)
    ix.close()


def test_ogg_index_single_class_fields(cuda, encoded):
    import vorbis_aotuv_lancer_amd as v
    ix = v.OggIndex([encoded[0], encoded[2]])
    assert ix.file_channels.tolist() == [2, 2] and ix.file_rates.tolist() == [44100, 44100]
    ix.close()
    ix = v.OggIndex([encoded[1]], one_decoder=True)                    # one class through the mixed path
    assert (ix.channels, ix.rate) == (1, 8000)
    ix.close()


def test_cut_ranges_over_two_classes(cuda, encoded):
    import vorbis_aotuv_lancer_amd as v
    ix = v.OggIndex(encoded, one_decoder=True)
    f = np.array([0, 1, 2, 4, 3, 1])
    starts = np.array([1000, 300, 12345, 100, 50, 9000], np.int64)
    lengths = np.array([5000, 4000, 8000, 2000, 3000, 6000])
    clips, cs, cl, status = ix.cut_ranges(f, starts, lengths)
    assert status.tolist() == [0] * 6 and np.array_equal(cs, starts) and np.array_equal(cl, lengths)
    pcm, got = ix.decode_ranges(f, cs, cl)
    assert np.array_equal(got, cl)
    for r, (clip, rate) in enumerate(v.decode_ogg(clips)):
        ch = int(ix.file_channels[f[r]])
        assert rate == ix.file_rates[f[r]] and tuple(clip.shape) == (ch, int(cl[r]))
        assert torch.equal(clip, pcm[r, :ch, :int(cl[r])]), r
    out = torch.zeros(sum(len(c) for c in clips) + 64, dtype=torch.uint8, device=cuda)
    off, os_, ol, st = ix.cut_ranges(f, starts, lengths, out=out)
    off, raw = off.cpu().tolist(), out.cpu().numpy().tobytes()
    assert st.cpu().tolist() == [0] * 7 and [raw[a:b] for a, b in zip(off[:-1], off[1:])] == clips
    assert os_.cpu().tolist() == cs.tolist() and ol.cpu().tolist() == cl.tolist()
    ix.close()


def test_refusals(cuda, corpus, encoded):
    """nothing is enqueued: the output keeps its fill"""
    v, classes, ds, streams, at = corpus
    tuples = [as_stream(pk) for _, pk in streams[:2]]
    md, store = open_mixed(v, classes, ds, streams[:2], 64)
    with pytest.raises(ValueError, match="one class id per stream"):
        v.RangeStore(md, tuples, classes=[0])
    for bad in (len(ds), -1):
        with pytest.raises(v.VbmError, match="class id"):
            v.RangeStore(md, tuples, classes=[0, bad])
    data, offs, gp, eo, first = R.csr(streams[:2])
    t = [torch.from_numpy(a).to(cuda) for a in (data, offs, gp, eo)]
    with pytest.raises(v.VbmError, match="class id"):
        v.RangeStore.from_device(md, *t, stream_packets=first, classes=[len(ds), 0])
    with pytest.raises(v.VbmError, match="class id"):
        v.decode_index_device(md, *t, stream_packets=first, classes=[0, len(ds)])
    one = v.Decoder(ds[0], 1, 64)
    with pytest.raises(v.VbmError, match="vbm_decoder_create_mixed"):
        v.RangeStore(one, tuples[:1], classes=[0])
    with pytest.raises(v.VbmError, match="vbm_decoder_create_mixed"):
        v.decode_index_device(one, *t, stream_packets=first, classes=[0, 0])
    single = v.RangeStore(one, tuples[:1])
    other, other_store = open_mixed(v, classes, ds, streams[:2], 64)
    pcm = torch.full((1, md.channels, 64), M.FILL_PLAYER, dtype=torch.float32, device=cuda)
    for dec, st in ((md, other_store), (other, store), (md, single)):
        with pytest.raises(v.VbmError, match="mixed"):
            dec.synthesis_ranges(st, [0], [0], [64], out=pcm)
    with pytest.raises(v.VbmError, match="another decoder"):
        one.synthesis_ranges(store, [0], [0], [64], out=pcm[:, :1])
    torch.cuda.synchronize()
    assert (pcm == M.FILL_PLAYER).all()
    _, got = md.synthesis_ranges(store, [0], [0], [64], out=pcm)        # the decoder and its store still work
    assert got.tolist() == [64] and (pcm[0, 0] != M.FILL_PLAYER).all() and (pcm[0, 1:] == M.FILL_PLAYER).all()
    for x in (single, one, other_store, other, store, md):
        x.close()
    ix = v.OggIndex(encoded[:2], one_decoder=True, halfrate=True)
    with pytest.raises(ValueError, match="full-rate"):
        ix.cut_ranges([0], [0], [100])
    ix.close()
