"""The device decoder on streams this project's encoder never writes: unpack and spectrum bit for bit against the
independent model (tests/vorbis_model.py) on the generated corpus, PCM of every block-size pair within the project's
bound of a float64 IMDCT + float64 Vorbis window + overlap-add, the runs and ranges paths against the stepwise one on
synthetic setups, and batches whose row x channel counts do not fill the IMDCT kernels' groups.  The PCM of the
block-size pairs, of those batches and of one mono stream alone is also compared bit for bit with the oracle's scalar
inverse MDCT (tests/decode_calls.py: check_pcm_exact)."""
import numpy as np
import pytest

from tests import vorbis_model as vm
from tests.decode_calls import (against_model, batch_inputs, check, check_pcm_bound, check_pcm_exact, ranges,
                                rows_tensor, runs_call, stepwise)
from tests.decode_packets import NAMES, RUNS, as_stream, family, fromdB, with_failed_packets

PAIR_IDS = [f"{a}_{b}" for a, b in vm.PAIRS]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(vm.CORPUS)), ids=NAMES)
def test_device_unpack_and_spectrum_equal_the_model(cuda, k):
    """every corpus packet of the family as a row of a fresh stream, in one call"""
    import vorbis_aotuv_lancer_amd as v
    _, _, h, _, rows, _, bad = family(k)
    assert not bad, bad[:3]                                     # host unpack = model (the CPU test's statement)
    ds = v.DecodeSetup(h)
    dec = v.Decoder(ds, len(rows), len(rows))
    pk, nb = rows_tensor([p for _, p, _ in rows], cuda)
    pcm, samples, status = dec.synthesis_batch(list(range(len(rows))), pk, nb)
    samples, status = samples.cpu().numpy(), status.cpu().numpy()
    assert not samples.any()                                    # the first packet of a stream returns nothing
    against_model(dec, [r for _, _, r in rows], status, samples, NAMES[k])
    dec.close()
    ds.close()


def decode_steps(v, ds, model, streams, cuda, what):
    """streams of equal length, one packet per stream per call -> the step lists check_pcm_bound takes; every step's
    intermediates are compared with the model on the way"""
    S, T = len(streams), len(streams[0])
    dec = v.Decoder(ds, S, S)
    pcm_steps, spec_steps, info_steps, samples_steps = [], [], [], []
    for t in range(T):
        pk, nb, gp, eo = batch_inputs([streams[s][t] for s in range(S)], cuda)
        pcm, samples, status = dec.synthesis_batch(list(range(S)), pk, nb, granulepos=gp, eos=eo)
        samples, status = samples.cpu().numpy(), status.cpu().numpy()
        got = against_model(dec, [model.decode(streams[s][t][0]) for s in range(S)], status, samples, f"{what} step {t}")
        assert not status.any()
        pcm_steps.append(pcm.cpu().numpy())
        spec_steps.append(got["spectrum"])
        info_steps.append(got["info"])
        samples_steps.append(samples)
    dec.close()
    return pcm_steps, spec_steps, info_steps, samples_steps


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(15), ids=PAIR_IDS)
def test_pcm_of_every_block_size_pair_is_within_the_bound(oracle, cuda, k):
    """Streams whose block-size sequence has every transition; stream 1's lW / nW bits contradict its neighbours (the
    decoder must go by the real previous block); the last packet is trimmed by its granule position.  The reference
    overlap-add uses the Vorbis window in float64, not the product's table.  Bound: the project's 1e-5 of the step's
    float64 peak; every peak is >= 1e-3, so the bound's floor never applies.  The same steps equal the oracle's scalar
    inverse MDCT + float32 overlap-add with the product's window tables bit for bit (check_pcm_exact)."""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(k)
    h = vm.pack_headers(setup, coding)
    ds = v.DecodeSetup(h)
    assert tuple(ds.blocksizes) == vm.PAIRS[k]
    model = vm.Model(setup, fromdB())
    streams = vm.pcm_streams(model, 7000 + k)
    steps = decode_steps(v, ds, model, streams, cuda, PAIR_IDS[k])
    # the block-size sequence really has the four transitions, whatever the packets' own lW / nW bits say
    for s, seq in enumerate(vm.SEQUENCES):
        W = [int(steps[2][t][s][1]) for t in range(len(seq))]
        if len({md[0] for md in setup["modes"]}) == 2:
            assert W == [int(c == "L") for c in seq]
            assert {(a, b) for a, b in zip(W, W[1:])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    total = [sum(int(steps[3][t][s]) for t in range(len(streams[s]))) for s in range(len(streams))]
    assert total == [pk[-1][1] for pk in streams]              # the granule position of the last packet
    win = [vm.vorbis_window64(ds.blocksizes[0] // 2), vm.vorbis_window64(ds.blocksizes[1] // 2)]
    peaks = []
    worst = check_pcm_bound(ds, streams, *steps, win=win, peaks=peaks)
    assert min(peaks) >= 1e-3, min(peaks)
    print(f"\nblock sizes {PAIR_IDS[k]}, {ds.channels} ch: max |pcm - float64 reference| / peak = {worst:.3g} "
          f"(peaks {min(peaks):.3g} .. {max(peaks):.3g})")
    exact = check_pcm_exact(oracle, ds, streams, *steps)
    print(f"block sizes {PAIR_IDS[k]}: {exact} steps x streams equal the scalar inverse MDCT bit for bit")
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", RUNS, ids=[n for n, _ in RUNS])
def test_runs_and_ranges_equal_the_stepwise_decode(cuda, name, k):
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(k)
    want_type = {"res0": 0, "res2": 2, "res1_3modes": 1}.get(name)
    if want_type is not None:
        assert want_type in {r["type"] for r in setup["residues"]}
    if name.startswith("pair"):
        assert setup["blocksizes"][0] == setup["blocksizes"][1]
    h = vm.pack_headers(setup, coding)
    ds = v.DecodeSetup(h)
    model = vm.Model(setup, fromdB())
    streams = with_failed_packets(vm.pcm_streams(model, 8000 + k), h, len(setup["modes"]), model.modebits)
    want = stepwise(v, ds, streams, cuda)
    assert all(any(st) for _, _, st in want)                   # the failed packets are inside
    for pk, (pcm, samples, status) in zip(streams, want):
        st, sm, out_start, total = v.decode_index(ds, *as_stream(pk))
        assert list(st) == status and list(sm) == samples and total == pcm.shape[1] > 0
        assert list(out_start) == [int(x) for x in np.cumsum([0] + samples[:-1])]
    # synthesis_runs: every stream whole, in one call
    P = sum(len(pk) for pk in streams)
    dec = v.Decoder(ds, len(streams), P)
    ids = list(range(len(streams)))[::-1]
    pcm, rs, sm, st = runs_call(dec, ids, [streams[i] for i in ids], cuda)
    pcm, rs, sm, st = pcm.cpu().numpy(), rs.cpu().numpy(), sm.cpu().tolist(), st.cpu().tolist()
    at = 0
    for r, i in enumerate(ids):
        c = len(streams[i])
        assert np.array_equal(pcm[r, :, :rs[r]], want[i][0]), f"{name}: run of stream {i}"
        assert sm[at:at + c] == want[i][1] and st[at:at + c] == want[i][2]
        at += c
    # synthesis_ranges: whole streams, and windows inside them
    store = v.RangeStore(dec, [as_stream(pk) for pk in streams])
    lin = [w[0] for w in want]
    assert list(store.totals) == [x.shape[1] for x in lin]
    rids = list(range(len(streams)))
    got = ranges(dec, store, rids, [0] * len(rids), [x.shape[1] for x in lin])
    check(lin, rids, [0] * len(rids), [x.shape[1] for x in lin], *got, what=f"{name} whole")
    rng = np.random.default_rng(9)
    rids = [int(i) for i in rng.integers(0, len(streams), 24)]
    starts = [int(rng.integers(0, lin[i].shape[1])) for i in rids]
    lengths = [int(rng.integers(1, 3000)) for _ in rids]
    got = ranges(dec, store, rids, starts, lengths)
    check(lin, rids, starts, lengths, *got, what=f"{name} windows")
    store.close()
    dec.close()
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bs,nshort,nlong", [((256, 1024), 3, 5), ((512, 2048), 5, 3), ((256, 512), 5, 3),
                                             ((1024, 1024), 3, 0)])
def test_batches_that_do_not_fill_the_imdct_groups(oracle, cuda, bs, nshort, nlong):
    """7 channels: 3 or 5 rows of a block size are 21 or 35 blocks, no multiple of the 8 / 4 / 2 blocks a wavefront
    takes at 256 / 512 / 1024; both block sizes in one call"""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.gen_setup(3000 + bs[0] + bs[1], ch=7, bs=bs, res_types=(1, 2), coupling="pairs", min_exp=0,
                                 res_kw=dict(bad_classwords=False, masks=[1, 3, 7]))
    h = vm.pack_headers(setup, coding)
    ds = v.DecodeSetup(h)
    model = vm.Model(setup, fromdB())
    seqs = ["SSSS"] * nshort + ["LLLL"] * nlong
    streams = vm.pcm_streams(model, 31, sequences=seqs)
    steps = decode_steps(v, ds, model, streams, cuda, f"{bs}")
    win = [vm.vorbis_window64(bs[0] // 2), vm.vorbis_window64(bs[1] // 2)]
    peaks = []
    worst = check_pcm_bound(ds, streams, *steps, win=win, peaks=peaks)
    assert min(peaks) >= 1e-3
    print(f"\n7 ch {bs}, {nshort} short + {nlong} long rows: max |pcm - float64 reference| / peak = {worst:.3g}")
    exact = check_pcm_exact(oracle, ds, streams, *steps)
    print(f"7 ch {bs}: {exact} steps x streams equal the scalar inverse MDCT bit for bit")
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("halfrate", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("bs", [(256, 2048), (512, 4096)], ids=["256_2048", "512_4096"])
def test_one_mono_stream_alone_equals_the_scalar_inverse_mdct(oracle, cuda, bs, halfrate):
    """the smallest launch: one mono stream, so one block per call.  The wavefront group of k_imdct holds 1 of its
    16 / 8 / 4 / 2 / 1 blocks and every other slot takes the zero path.  A sequence with all four transitions, decoded
    stepwise, bit for bit against the scalar inverse MDCT + float32 overlap-add"""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.gen_setup(4000 + bs[0] + bs[1], ch=1, bs=bs, res_types=(1, 2), min_exp=0,
                                 res_kw=dict(bad_classwords=False, masks=[1, 3, 7]))
    ds = v.DecodeSetup(vm.pack_headers(setup, coding))
    assert tuple(ds.blocksizes) == bs and ds.channels == 1
    model = vm.Model(setup, fromdB())
    streams = vm.pcm_streams(model, 41, sequences=[vm.SEQUENCES[0]])
    assert len(streams) == 1
    S, T = 1, len(streams[0])
    dec = v.Decoder(ds, S, S, halfrate=halfrate)
    pcm_steps, spec_steps, info_steps, samples_steps = [], [], [], []
    for t in range(T):
        p = streams[0][t][0]
        pk, nb, gp, eo = batch_inputs([streams[0][t]], cuda)
        pcm, samples, status = dec.synthesis_batch([0], pk, nb, granulepos=gp, eos=eo)
        assert not status.cpu().numpy().any()
        r = model.decode(p)
        spec = dec.fetch("spectrum").cpu().numpy()
        assert r["status"] == 0 and spec[0].tobytes() == r["spectrum"].tobytes(), t
        pcm_steps.append(pcm.cpu().numpy())
        spec_steps.append(spec)
        info_steps.append(dec.fetch("info").cpu().numpy())
        samples_steps.append(samples.cpu().numpy())
    dec.close()
    W = [int(i[0][1]) for i in info_steps]
    assert {(a, b) for a, b in zip(W, W[1:])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    peak = max(float(np.abs(p[0, :, :int(n[0])]).max()) for p, n in zip(pcm_steps, samples_steps) if n[0])
    assert peak >= 1e-3                       # loud packets: the comparison is not one of zeros
    exact = check_pcm_exact(oracle, ds, streams, pcm_steps, spec_steps, info_steps, samples_steps, halfrate=halfrate)
    assert exact >= T - 2                     # every step but the first (and a last one trimmed to nothing) returns PCM
    ds.close()
