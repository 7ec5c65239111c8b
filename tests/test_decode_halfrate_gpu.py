"""Half-rate decoding on the MI355X (Decoder(..., halfrate=True); the reference's vorbis_synthesis_halfrate): PCM of
every block-size pair and of a real stream within the project's bound of a float64 reference — IMDCT of half the block
size over the lower half of the float32 spectrum, the Vorbis window of half the size in float64, overlap-add — and bit
for bit against the oracle's scalar inverse MDCT of that size + float32 overlap-add (check_pcm_exact), batches
that do not fill the 128-point transform's groups, runs and ranges bit for bit against the stepwise half-rate decode,
and a full-rate and a half-rate decoder side by side."""
import numpy as np
import pytest
import torch

from tests import vorbis_model as vm
from tests.decode_calls import (batch_inputs, check, check_pcm_bound, check_pcm_exact, ranges, rows_tensor, runs_call,
                                step_rows, stepwise)
from tests.decode_packets import RUNS, as_stream, dump_packets, fromdB, with_failed_packets

PAIR_IDS = [f"{a}_{b}" for a, b in vm.PAIRS]


def as_info(W_steps):
    """the step lists' block flags as the info rows check_pcm_bound and check_pcm_exact read"""
    return [[(0, int(W)) for W in row] for row in W_steps]


def check_halfrate_bound(ds, streams, spec_steps, W_steps, pcm_steps, samples_steps, peaks):
    """check_pcm_bound at half rate, the reference's spectra those of spec_steps[t][s] ([ch][bs1/2] float32, full rate)
    and its windows the Vorbis window of half each block size in float64 -> worst error / peak"""
    win = [vm.vorbis_window64(ds.blocksizes[0] // 4), vm.vorbis_window64(ds.blocksizes[1] // 4)]
    return check_pcm_bound(ds, streams, pcm_steps, spec_steps, as_info(W_steps), samples_steps, win=win, peaks=peaks,
                           halfrate=True)


def model_steps(v, ds, model, streams, cuda):
    """streams of equal length, one packet per stream per call on a half-rate decoder; the reference's spectra are the
    model's (vm.Model.decode).  The decoder's own "spectrum" is the full-rate one and must equal it bit for bit."""
    S, T = len(streams), len(streams[0])
    dec = v.Decoder(ds, S, S, halfrate=True)
    assert dec.halfrate and dec.row == ds.blocksizes[1] // 4
    spec_steps, W_steps, pcm_steps, samples_steps = [], [], [], []
    for t in range(T):
        pk, nb, gp, eo = batch_inputs([streams[s][t] for s in range(S)], cuda)
        pcm, samples, status = dec.synthesis_batch(list(range(S)), pk, nb, granulepos=gp, eos=eo)
        assert tuple(pcm.shape) == (S, ds.channels, ds.blocksizes[1] // 4)
        assert not status.cpu().numpy().any()
        res = [model.decode(streams[s][t][0]) for s in range(S)]
        spec = dec.fetch("spectrum").cpu().numpy()
        for s in range(S):
            assert res[s]["status"] == 0 and spec[s].tobytes() == res[s]["spectrum"].tobytes(), (t, s)
        spec_steps.append([r["spectrum"] for r in res])
        W_steps.append([r["info"][1] for r in res])
        pcm_steps.append(pcm.cpu().numpy())
        samples_steps.append(samples.cpu().numpy())
    dec.close()
    return spec_steps, W_steps, pcm_steps, samples_steps


def exact_halfrate(oracle, ds, streams, spec_steps, W_steps, pcm_steps, samples_steps):
    """check_pcm_exact at half rate on the step lists of this file -> steps x streams compared"""
    return check_pcm_exact(oracle, ds, streams, pcm_steps, spec_steps, as_info(W_steps), samples_steps, halfrate=True)


def assert_samples_equal_the_index(v, ds, streams, samples_steps):
    totals = []
    for s, pk in enumerate(streams):
        st, sm, _, total = v.decode_index(ds, *as_stream(pk), halfrate=True)
        assert not st.any()
        assert [int(samples_steps[t][s]) for t in range(len(pk))] == list(sm), f"stream {s}"
        totals.append(total)
    return totals


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(15), ids=PAIR_IDS)
def test_halfrate_pcm_of_every_block_size_pair_is_within_the_bound(oracle, cuda, k):
    """Transforms of 128 .. 2048 points, every block-size transition at each; the last packet is trimmed by its
    granule position (37 full-rate samples: 18 output samples).
    Measured on MI355X, max |pcm - float64 reference| / peak over the 15 pairs: see DESIGN.md §9c."""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(k)
    ds = v.DecodeSetup(vm.pack_headers(setup, coding))
    assert tuple(ds.blocksizes) == vm.PAIRS[k]
    model = vm.Model(setup, fromdB())
    streams = vm.pcm_streams(model, 7000 + k)
    spec_steps, W_steps, pcm_steps, samples_steps = model_steps(v, ds, model, streams, cuda)
    if len({md[0] for md in setup["modes"]}) == 2:
        for s in range(len(streams)):
            W = [int(W_steps[t][s]) for t in range(len(streams[s]))]
            assert {(a, b) for a, b in zip(W, W[1:])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    totals = assert_samples_equal_the_index(v, ds, streams, samples_steps)
    assert totals == [(pk[-1][1] + 37) // 2 - 18 for pk in streams]        # tests/test_decode_halfrate_cpu.py
    peaks = []
    worst = check_halfrate_bound(ds, streams, spec_steps, W_steps, pcm_steps, samples_steps, peaks)
    assert min(peaks) >= 1e-3, min(peaks)
    print(f"\nhalf rate, block sizes {PAIR_IDS[k]}, {ds.channels} ch: max |pcm - float64 reference| / peak = "
          f"{worst:.3g} (peaks {min(peaks):.3g} .. {max(peaks):.3g})")
    exact = exact_halfrate(oracle, ds, streams, spec_steps, W_steps, pcm_steps, samples_steps)
    print(f"half rate, block sizes {PAIR_IDS[k]}: {exact} steps x streams equal the scalar inverse MDCT bit for bit")
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bs,nshort,nlong", [((256, 2048), 3, 5), ((256, 2048), 5, 3), ((256, 256), 3, 0),
                                             ((256, 256), 5, 0)])
def test_halfrate_batches_that_do_not_fill_the_imdct_groups(oracle, cuda, bs, nshort, nlong):
    """7 channels: 3 or 5 rows of a block size are 21 or 35 blocks, no multiple of the 16 blocks a wavefront takes at
    128 points (or of the 2 at 1024); both block sizes in one call"""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.gen_setup(3000 + bs[0] + bs[1], ch=7, bs=bs, res_types=(1, 2), coupling="pairs", min_exp=0,
                                 res_kw=dict(bad_classwords=False, masks=[1, 3, 7]))
    ds = v.DecodeSetup(vm.pack_headers(setup, coding))
    assert tuple(ds.blocksizes) == bs and ds.channels == 7
    model = vm.Model(setup, fromdB())
    streams = vm.pcm_streams(model, 31, sequences=["SSSS"] * nshort + ["LLLL"] * nlong)
    spec_steps, W_steps, pcm_steps, samples_steps = model_steps(v, ds, model, streams, cuda)
    if nlong:
        assert sorted(int(w) for w in W_steps[0]) == [0] * nshort + [1] * nlong
    assert_samples_equal_the_index(v, ds, streams, samples_steps)
    peaks = []
    worst = check_halfrate_bound(ds, streams, spec_steps, W_steps, pcm_steps, samples_steps, peaks)
    assert min(peaks) >= 1e-3
    print(f"\nhalf rate, 7 ch {bs}, {nshort} short + {nlong} long rows: max |pcm - float64 reference| / peak = "
          f"{worst:.3g}")
    exact = exact_halfrate(oracle, ds, streams, spec_steps, W_steps, pcm_steps, samples_steps)
    print(f"half rate, 7 ch {bs}: {exact} steps x streams equal the scalar inverse MDCT bit for bit")
    ds.close()


def decode_in_runs(dec, streams, cuts, dev, single=()):
    """every stream cut at the packet indices `cuts`, one synthesis_runs call per piece over all streams; pieces whose
    number is in `single` go packet by packet through synthesis_batch instead -> per stream (pcm, samples, status)"""
    S = len(streams)
    dec.reset()
    pcm, samp, stat = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    edges = [0] + list(cuts) + [max(len(s) for s in streams)]
    for j, (a, b) in enumerate(zip(edges, edges[1:])):
        if j in single:
            for t in range(a, b):
                ids = [s for s in range(S) if t < len(streams[s])]
                step_rows(dec, ids, [streams[s][t] for s in ids], dev, pcm, samp, stat)
            continue
        ids = [s for s in range(S) if a < len(streams[s])]
        runs = [streams[s][a:b] for s in ids]
        p, rs, sm, st = runs_call(dec, ids, runs, dev)
        assert p.shape[2] == max(len(r) for r in runs) * dec.blocksizes[1] // 4
        p, rs, sm, st = p.cpu().numpy(), rs.cpu().numpy(), sm.cpu().tolist(), st.cpu().tolist()
        at = 0
        for r, s in enumerate(ids):
            c = len(runs[r])
            pcm[s].append(p[r, :, :rs[r]])
            samp[s] += sm[at:at + c]
            stat[s] += st[at:at + c]
            at += c
    return [(np.concatenate(pcm[s], axis=1), samp[s], stat[s]) for s in range(S)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", RUNS, ids=[n for n, _ in RUNS])
def test_halfrate_runs_and_ranges_equal_the_stepwise_decode(cuda, name, k):
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(k)
    h = vm.pack_headers(setup, coding)
    ds = v.DecodeSetup(h)
    model = vm.Model(setup, fromdB())
    streams = with_failed_packets(vm.pcm_streams(model, 8000 + k), h, len(setup["modes"]), model.modebits)
    want = stepwise(v, ds, streams, cuda, halfrate=True)
    assert all(any(st) for _, _, st in want)                   # the failed packets are inside
    for pk, (pcm, samples, status) in zip(streams, want):
        st, sm, out_start, total = v.decode_index(ds, *as_stream(pk), halfrate=True)
        assert list(st) == status and list(sm) == samples and total == pcm.shape[1] > 0
        assert total == (pk[-1][1] + 37) // 2 - 18
    P = sum(len(pk) for pk in streams)
    dec = v.Decoder(ds, len(streams), P, halfrate=True)
    # any split into runs and single-packet calls gives the same bits
    for cuts, single in (((), ()), ((1, 5, 7), ()), ((3, 6, 9), (1,)), ((2, 4, 11), (0, 2))):
        got = decode_in_runs(dec, streams, cuts, cuda, single)
        for s in range(len(streams)):
            assert got[s][2] == want[s][2] and got[s][1] == want[s][1], f"{name} cuts {cuts}: stream {s}"
            assert got[s][0].dtype == np.float32 and np.array_equal(got[s][0], want[s][0]), \
                f"{name} cuts {cuts}: pcm of stream {s}"
    with pytest.raises(v.VbmError):                            # the stride is checked at the decoder's rate
        dec.synthesis_runs([0], [2], torch.zeros(1, dtype=torch.uint8, device=cuda),
                           torch.zeros(3, dtype=torch.int64, device=cuda), pcm_stride=2 * (ds.blocksizes[1] // 4) - 1)
    # ranges: the store takes its index at the decoder's rate
    store = v.RangeStore(dec, [as_stream(pk) for pk in streams])
    lin = [w[0] for w in want]
    assert store.halfrate and list(store.totals) == [x.shape[1] for x in lin]
    S = len(streams)
    rids = list(range(S))
    whole = ranges(dec, store, rids, [0] * S, [x.shape[1] for x in lin])
    check(lin, rids, [0] * S, [x.shape[1] for x in lin], *whole, what=f"{name} whole")
    rng = np.random.default_rng(9)
    rids = [int(i) for i in rng.integers(0, S, 24)]
    starts = [int(rng.integers(0, lin[i].shape[1])) for i in rids]
    lengths = [int(2 * rng.integers(0, 700) + 1) for _ in rids]          # odd lengths
    # at 0, ending exactly at the end, reaching past the end, starting at and past the end
    for i in range(S):
        T = lin[i].shape[1]
        rids += [i] * 5
        starts += [0, T - 33, T - 10, T, T + 5]
        lengths += [77, 33, 101, 9, 9]
    got = ranges(dec, store, rids, starts, lengths)
    check(lin, rids, starts, lengths, *got, what=f"{name} windows")
    # a window cut into pieces by a small max_batch equals the uncut one
    small = v.Decoder(ds, 1, 3, halfrate=True)
    store3 = v.RangeStore(small, [as_stream(pk) for pk in streams])
    got3 = ranges(small, store3, rids, starts, lengths)
    assert np.array_equal(got3[0], got[0]) and list(got3[1]) == list(got[1])
    store3.close()
    small.close()
    store.close()
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_halfrate_of_a_real_stream(oracle, cuda):
    """the first 200 packets of the reference encoder's 44.1 kHz stereo q5 dump as four streams of 50; the float64
    reference is built from the spectrum a full-rate decoder fetches for the same packets"""
    import vorbis_aotuv_lancer_amd as v
    ds = v.DecodeSetup(v.header_packets(v.Setup(2, 44100, 0.5)))
    packets = dump_packets("ref_scalar_2ch_44100_q05_20s.pkt")[:200]
    S, T = 4, 50
    streams = [[(p, -1, 0) for p in packets[s * T:(s + 1) * T]] for s in range(S)]
    full = v.Decoder(ds, S, S)
    half = v.Decoder(ds, S, S, halfrate=True)
    assert (full.rate, half.rate) == (44100, 22050) and isinstance(half.rate, int)
    spec_steps, W_steps, pcm_steps, samples_steps, full_samples, full_pcm = [], [], [], [], [], []
    for t in range(T):
        pk, nb = rows_tensor([streams[s][t][0] for s in range(S)], cuda)
        fp, fs, st = full.synthesis_batch(list(range(S)), pk, nb)
        assert not st.cpu().numpy().any()
        full_pcm.append(fp.cpu().numpy())
        spec_steps.append(full.fetch("spectrum").cpu().numpy())
        W_steps.append(full.fetch("info").cpu().numpy()[:, 1])
        full_samples.append(fs.cpu().numpy())
        pcm, samples, st = half.synthesis_batch(list(range(S)), pk, nb)
        assert not st.cpu().numpy().any()
        pcm_steps.append(pcm.cpu().numpy())
        samples_steps.append(samples.cpu().numpy())
    assert {int(w) for ws in W_steps for w in ws} == {0, 1}                 # both block sizes: 128 and 1024 points
    assert all(np.array_equal(2 * samples_steps[t], full_samples[t]) for t in range(T))
    assert_samples_equal_the_index(v, ds, streams, samples_steps)
    peaks = []
    worst = check_halfrate_bound(ds, streams, spec_steps, W_steps, pcm_steps, samples_steps, peaks)
    print(f"\nhalf rate, 2ch 44100 q0.5 reference stream: max |pcm - float64 reference| / peak = {worst:.3g} "
          f"(peaks {min(peaks):.3g} .. {max(peaks):.3g})")
    exact = exact_halfrate(oracle, ds, streams, spec_steps, W_steps, pcm_steps, samples_steps)
    # the full-rate decoder beside it, on the same packets and spectra
    exact_full = check_pcm_exact(oracle, ds, streams, full_pcm, spec_steps, as_info(W_steps), full_samples)
    print(f"reference stream: {exact} steps x streams at half rate and {exact_full} at full rate equal the scalar inverse "
          f"MDCT bit for bit")
    full.close()
    half.close()
    ds.close()


@pytest.mark.gpu
def test_full_rate_and_half_rate_decoders_side_by_side(cuda):
    """one DecodeSetup, calls interleaved: the full-rate PCM is that of a full-rate decoder alone, and a restart on the
    half-rate decoder gives the fresh-stream output again"""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(3)                            # 256 / 2048
    ds = v.DecodeSetup(vm.pack_headers(setup, coding))
    model = vm.Model(setup, fromdB())
    streams = vm.pcm_streams(model, 9100)
    S, T = len(streams), len(streams[0])

    def step(dec, t):
        pk, nb, gp, eo = batch_inputs([streams[s][t] for s in range(S)], cuda)
        pcm, n, st = dec.synthesis_batch(list(range(S)), pk, nb, granulepos=gp, eos=eo)
        assert not st.cpu().numpy().any()
        n = n.cpu().numpy()
        return [pcm[s, :, :n[s]].cpu().numpy() for s in range(S)]

    alone = v.Decoder(ds, S, S)
    want_full = [step(alone, t) for t in range(T)]
    alone.close()
    want_half = stepwise(v, ds, streams, cuda, halfrate=True)
    full, half = v.Decoder(ds, S, S), v.Decoder(ds, S, S, halfrate=True)
    assert not full.halfrate and half.halfrate
    got_half = [[] for _ in range(S)]
    for t in range(T):
        h = step(half, t)
        f = step(full, t)
        for s in range(S):
            assert np.array_equal(f[s], want_full[t][s]), f"full-rate step {t} stream {s}"
            assert f[s].shape[1] == 2 * h[s].shape[1] or t == T - 1
            got_half[s].append(h[s])
    for s in range(S):
        assert np.array_equal(np.concatenate(got_half[s], axis=1), want_half[s][0])
    # restart: the half-rate decoder's streams decode the same packets again as fresh streams
    half.restart_streams(list(range(S)))
    again = [[] for _ in range(S)]
    for t in range(T):
        h = step(half, t)
        for s in range(S):
            again[s].append(h[s])
    for s in range(S):
        assert np.array_equal(np.concatenate(again[s], axis=1), want_half[s][0])
    full.close()
    half.close()
    ds.close()
