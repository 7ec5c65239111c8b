"""Runs of consecutive packets per stream (Decoder.synthesis_runs) and whole Ogg files (decode_ogg) on the MI355X.
Every check is bit-for-bit (np.array_equal on float32) against the stepwise path, one packet per stream per call
through synthesis_batch."""
import numpy as np
import pytest
import torch

from tests.decode_calls import (Collect, assert_same, device_encode, encode_chunked, encoded, rows_tensor, runs_call,
                                runs_inputs, stepwise)
from tests.decode_packets import EINVAL, ENOTAUDIO, pack_setup
from tests.signals import burst_signal, gen_windowed_sine


CLASSES = ["mode_1ch_44100_q0.5.vpk", "mode_2ch_44100_q0.1.vpk", "mode_2ch_44100_q0.5.vpk", "mode_6ch_48000_q0.5.vpk",
           "mode_8ch_44100_q0.5.vpk", "mode_2ch_96000_q0.5.vpk", "mode_2ch_44100_b128000.vpk",
           "mode_2ch_44100_q-0.1.vpk", "mode_2ch_22050_q0.5.vpk"]


@pytest.mark.gpu
@pytest.mark.parametrize("pack", CLASSES)
def test_whole_stream_in_one_call_equals_stepwise(cuda, pack):
    import vorbis_aotuv_lancer_amd as v
    setup, _ = pack_setup(v, pack)
    pk = encoded(v, setup, 2.0, 41, cuda)
    ds = v.DecodeSetup(v.header_packets(setup))
    want = stepwise(v, ds, [pk], cuda)[0]
    dec = v.Decoder(ds, 3, len(pk))
    col = Collect(3)
    col.add_runs([2], [pk], runs_call(dec, [2], [pk], cuda))
    got = col.result(2)
    assert_same(got, want, pack)
    assert sum(got[1]) == got[0].shape[1] > 0 and max(got[2]) == 0
    if pack == "mode_2ch_44100_q-0.1.vpk":
        assert ds.blocksizes[1] == 4096
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_split_invariance(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    pk = encoded(v, setup, 3.0, 42, cuda)
    P = len(pk)
    ds = v.DecodeSetup(v.header_packets(setup))
    want = stepwise(v, ds, [pk], cuda)[0]
    for size in (1, 3, 17, P):
        dec = v.Decoder(ds, 1, size)
        col = Collect(1)
        for a in range(0, P, size):
            col.add_runs([0], [pk[a:a + size]], runs_call(dec, [0], [pk[a:a + size]], cuda))
        assert_same(col.result(0), want, f"runs of {size}")
        dec.close()
    # stepwise, then runs, then stepwise again, then a run of 0 and the rest as one run
    dec = v.Decoder(ds, 1, P)
    col = Collect(1)
    cuts = [0, 5, 30, 36, 36, P]
    for i in range(len(cuts) - 1):
        seg = pk[cuts[i]:cuts[i + 1]]
        if i % 2 == 0 and seg:
            for p in seg:
                r, n = rows_tensor([p[0]], cuda)
                col.add_steps([0], dec.synthesis_batch([0], r, n, torch.tensor([p[1]], device=cuda),
                                                       torch.tensor([p[2]], dtype=torch.uint8, device=cuda)))
        else:
            col.add_runs([0], [seg], runs_call(dec, [0], [seg], cuda))
    assert_same(col.result(0), want, "mixed")
    dec.close()
    ds.close()


def unequal_streams(v, setup, cuda, S, seed):
    """S streams of 1 .. ~300 packets cut from a few encoded signals (the full ones end with eos)"""
    base = [encoded(v, setup, 7.5, seed + k, cuda) for k in range(3)]
    rng = np.random.default_rng(seed)
    out = []
    for s in range(S):
        b = base[s % 3]
        n = len(b) if s % 5 == 0 else int(rng.integers(1, len(b)))
        out.append(b[:n])
    out[1] = base[1][:1]
    return out


@pytest.mark.gpu
def test_many_streams_of_unequal_length(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    S = 40
    streams = unequal_streams(v, setup, cuda, S, 50)
    assert max(len(s) for s in streams) >= 250
    ds = v.DecodeSetup(v.header_packets(setup))
    want = stepwise(v, ds, streams, cuda)
    # one call, with runs of 0 (streams that take part with no packet) among the others
    P = sum(len(s) for s in streams)
    dec = v.Decoder(ds, S + 2, P)
    col = Collect(S + 2)
    ids = [S] + list(range(S)) + [S + 1]
    runs = [[]] + streams + [[]]
    out = runs_call(dec, ids, runs, cuda)
    col.add_runs(ids, runs, out)
    assert out[1][0].item() == 0 and out[1][-1].item() == 0
    for s in range(S):
        assert_same(col.result(s), want[s], f"one call, stream {s}")
    dec.close()
    # several calls that never wait for the host: random counts per stream and call (0 included), random order
    rng = np.random.default_rng(3)
    dec = v.Decoder(ds, S, 600)
    col = Collect(S)
    pos = [0] * S
    while any(pos[s] < len(streams[s]) for s in range(S)):
        ids, runs, budget = [], [], 600
        for s in rng.permutation(S):
            c = min(int(rng.integers(0, 40)), len(streams[s]) - pos[s], budget)
            if rng.random() < 0.3 and c:
                continue                                     # this stream sits this call out
            ids.append(int(s))
            runs.append(streams[s][pos[s]:pos[s] + c])
            pos[s] += c
            budget -= c
        col.add_runs(ids, runs, runs_call(dec, ids, runs, cuda))
    for s in range(S):
        assert_same(col.result(s), want[s], f"several calls, stream {s}")
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_failed_packets_inside_a_run(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    h = v.header_packets(setup)
    pk = encoded(v, setup, 2.0, 43, cuda)
    rng = np.random.default_rng(1)
    bad = list(pk)
    bad.insert(10, (h[2], -1, 0))                                          # a header packet
    bad.insert(20, (pk[19][0][:len(pk[19][0]) // 3], -1, 0))               # a truncated packet
    bad.insert(30, (rng.integers(0, 256, 200, dtype=np.uint8).tobytes(), -1, 0))   # garbage
    bad.insert(31, (b"", -1, 0))                                           # nothing
    bad.insert(0, (h[0], -1, 0))                                           # before the first audio packet
    ds = v.DecodeSetup(h)
    want = stepwise(v, ds, [bad], cuda)[0]
    assert want[2][11] == ENOTAUDIO and want[2][0] == ENOTAUDIO and sum(1 for s in want[2] if s) >= 3
    assert all(n == 0 for n, s in zip(want[1], want[2]) if s)
    for size in (len(bad), 7):
        dec = v.Decoder(ds, 1, size)
        col = Collect(1)
        for a in range(0, len(bad), size):
            col.add_runs([0], [bad[a:a + size]], runs_call(dec, [0], [bad[a:a + size]], cuda))
        assert_same(col.result(0), want, f"runs of {size}")
        dec.close()
    ds.close()


@pytest.mark.gpu
def test_granulepos_windowed_sine_is_2048_samples(cuda):
    """test/test.c's windowed sine, encoded with end of stream, decodes to exactly its 2048 samples through runs"""
    import vorbis_aotuv_lancer_amd as v
    for ch, rate, q in [(2, 44100, 0.5), (1, 44100, 0.1)]:
        setup = v.Setup(ch, rate, q)
        pk = device_encode(v, setup, np.repeat(gen_windowed_sine()[None, :], ch, axis=0), cuda)[0]
        ds = v.DecodeSetup(v.header_packets(setup))
        dec = v.Decoder(ds, 1, len(pk))
        col = Collect(1)
        col.add_runs([0], [pk], runs_call(dec, [0], [pk], cuda))
        got = col.result(0)
        assert got[0].shape == (ch, 2048)
        assert_same(got, stepwise(v, ds, [pk], cuda)[0])
        dec.close()
        ds.close()


@pytest.mark.gpu
def test_granulepos_trimmed_start_and_restart(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    pk = encoded(v, setup, 2.0, 44, cuda)
    # no granulepos before packet 4 (as on a page that closes later), and packet 4's lowered: the start is trimmed
    low = [(p, -1, e) for p, _, e in pk[:4]] + list(pk[4:])
    low[4] = (low[4][0], low[4][1] - 700, low[4][2])
    ds = v.DecodeSetup(v.header_packets(setup))
    want = stepwise(v, ds, [low], cuda)[0]
    plain = stepwise(v, ds, [pk], cuda)[0]
    assert sum(want[1]) < sum(plain[1])
    for size in (len(low), 2, 5):
        dec = v.Decoder(ds, 1, size)
        col = Collect(1)
        for a in range(0, len(low), size):
            col.add_runs([0], [low[a:a + size]], runs_call(dec, [0], [low[a:a + size]], cuda))
        assert_same(col.result(0), want, f"trimmed start, runs of {size}")
        dec.close()
    # restart_streams between runs behaves as between steps
    cut = 25
    want = stepwise(v, ds, [pk], cuda, restart_at={0: cut})[0]
    dec = v.Decoder(ds, 2, len(pk))
    col = Collect(2)
    col.add_runs([1, 0], [pk[:3], pk[:cut]], runs_call(dec, [1, 0], [pk[:3], pk[:cut]], cuda))
    dec.restart_streams([0])
    col.add_runs([0], [pk[cut:]], runs_call(dec, [0], [pk[cut:]], cuda))
    got = col.result(0)
    assert got[1][cut] == 0
    assert_same(got, want, "restart")
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_argument_errors(cuda):
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    setup = v.Setup(2, 44100, 0.5)
    pk = encoded(v, setup, 1.0, 45, cuda)
    ds = v.DecodeSetup(v.header_packets(setup))
    dec = v.Decoder(ds, 4, 8)
    data, offs, gp, eo, _ = runs_inputs([pk[:4], pk[4:8]], cuda)
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        dec.synthesis_runs([1, 1], [4, 4], data, offs)                         # duplicate ids
    data9, offs9, _, _, _ = runs_inputs([pk[:5], pk[5:9]], cuda)
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        dec.synthesis_runs([0, 1], [5, 4], data9, offs9)                       # P = 9 > max_batch = 8
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        dec.synthesis_runs([0, 1], [4, 4], data, offs, pcm_stride=4 * 1024 - 1)   # stride too small
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        dec.synthesis_runs([0, 4], [4, 4], data, offs)                         # id out of range
    cnt = np.array([-1, 9], np.int32)
    ids = np.array([0, 1], np.int32)
    out = torch.empty((2, 2, 9 * 1024), device=cuda)
    i32 = [torch.empty(9, dtype=torch.int32, device=cuda) for _ in range(3)]
    assert lib.vbm_synthesis_runs(dec._h, 2, ids.ctypes.data, cnt.ctypes.data, data.data_ptr(), offs.data_ptr(),
                                  data.numel(), None, None, out.data_ptr(), 9 * 1024, i32[0].data_ptr(),
                                  i32[1].data_ptr(), i32[2].data_ptr(), None) == EINVAL   # negative count
    # nothing was enqueued by the refused calls: the streams still start fresh
    col = Collect(4)
    col.add_runs([0, 1], [pk[:4], pk[4:8]], dec.synthesis_runs([0, 1], [4, 4], data, offs, granulepos=gp, eos=eo))
    want = stepwise(v, ds, [pk[:4], pk[4:8]], cuda)
    assert_same(col.result(0), want[0])
    assert_same(col.result(1), want[1])
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_full_size_runs_unsynchronised(cuda):
    """4096 stereo q0.5 streams x 32 packets per call, K distinct lead signals dealt round robin, calls back to back
    with no host synchronisation: every stream equals its lead, and the leads equal their stepwise decode"""
    import vorbis_aotuv_lancer_amd as v
    S, K, R, ch, rate = 4096, 8, 32, 2, 44100
    setup = v.Setup(ch, rate, 0.5)
    nsamp = 100 * 1024
    sigs = [burst_signal(ch, rate, nsamp, seed=900 + k, level=1.0 if k % 3 else 0.05) for k in range(K)]
    lead = [encode_chunked(v, setup, sigs[k], cuda) for k in range(K)]
    ds = v.DecodeSetup(v.header_packets(setup))
    want = stepwise(v, ds, lead, cuda)
    ncalls = min(len(x) for x in lead) // R
    assert ncalls >= 3
    half = ds.blocksizes[1] // 2
    inputs = []
    for c in range(ncalls):                              # every call's inputs on the device before the first call
        per = []
        for k in range(K):
            seg = lead[k][c * R:(c + 1) * R]
            b = b"".join(p[0] for p in seg)
            o = np.cumsum([0] + [len(p[0]) for p in seg]).astype(np.int64)
            per.append((np.frombuffer(b, np.uint8), o, [p[1] for p in seg], [p[2] for p in seg]))
        data, offs, gps, eos, base = [], [np.zeros(1, np.int64)], [], [], 0
        for s in range(S):
            b, o, g, e = per[s % K]
            data.append(b)
            offs.append(o[1:] + base)
            gps += g
            eos += e
            base += len(b)
        inputs.append((torch.from_numpy(np.concatenate(data)).to(cuda), torch.from_numpy(np.concatenate(offs)).to(cuda),
                       torch.tensor(gps, dtype=torch.int64, device=cuda), torch.tensor(eos, dtype=torch.uint8, device=cuda)))
    dec = v.Decoder(ds, S, S * R)
    ids = list(range(S))
    lead_of = torch.arange(S, device=cuda) % K
    mism = torch.zeros((), dtype=torch.int64, device=cuda)
    col = Collect(K)
    for c in range(ncalls):
        data, offs, gp, eo = inputs[c]
        pcm, rs, sm, st = dec.synthesis_runs(ids, [R] * S, data, offs, granulepos=gp, eos=eo, pcm_stride=R * half)
        mism += (pcm != pcm[lead_of]).flatten(1).any(dim=1).sum() + (rs != rs[lead_of]).sum()
        sm2, st2 = sm.view(S, R), st.view(S, R)
        mism += (sm2 != sm2[lead_of]).sum() + (st2 != 0).sum()
        col.add_runs(ids[:K], [[None] * R] * K, (pcm[:K].clone(), rs[:K].clone(), sm[:K * R].clone(), st[:K * R].clone()))
    torch.cuda.synchronize()
    assert int(mism) == 0
    for k in range(K):
        got = col.result(k)
        n = ncalls * R
        upto = sum(want[k][1][:n])
        assert got[2] == want[k][2][:n] and got[1] == want[k][1][:n], f"lead {k}"
        assert np.array_equal(got[0], want[k][0][:, :upto]), f"lead {k}"
    dec.close()
    ds.close()


def ogg_with_bad_setup(v, setup, packets):
    h = v.header_packets(setup)
    os_ = v.OggStream(7)
    os_.packetin(h[0], 0)
    os_.packetin(h[1], 0)
    os_.packetin(h[2][:40], 0)
    out = os_.pages(flush=True)
    for p, gp, e in packets:
        os_.packetin(p, gp, e)
    out += os_.pages(flush=True)
    os_.close()
    return b"".join(out)


@pytest.mark.gpu
def test_decode_ogg_two_setups(cuda, tmp_path):
    import vorbis_aotuv_lancer_amd as v
    setups = [v.Setup(2, 44100, 0.5), v.Setup(1, 44100, 0.1)]
    files, want = [], []
    for i in range(7):
        setup = setups[i % 2]
        pk = encoded(v, setup, 0.5 + 0.4 * i, 60 + i, cuda)
        blob = v.write_ogg(setup, [p[0] for p in pk], [(p[1], p[2]) for p in pk], serialno=i)
        if i == 3:
            path = tmp_path / "three.ogg"
            path.write_bytes(blob)
            files.append(str(path))
        else:
            files.append(blob)
        h, rp, rg, re_ = v.read_ogg(blob)
        ds = v.DecodeSetup(h)
        want.append((stepwise(v, ds, [list(zip(rp, rg, [int(e) for e in re_]))], cuda)[0][0], ds.rate))
        ds.close()
    for mp in (7, 4096):
        got = v.decode_ogg(files, max_packets=mp)
        assert len(got) == len(files)
        for i, ((pcm, rate), (wp, wr)) in enumerate(zip(got, want)):
            assert rate == wr and pcm.is_cuda and pcm.is_contiguous() and pcm.dtype == torch.float32
            assert np.array_equal(pcm.cpu().numpy(), wp), f"file {i}, max_packets {mp}"
    bad = ogg_with_bad_setup(v, setups[0], encoded(v, setups[0], 0.3, 70, cuda))
    with pytest.raises(v.VbmError, match="file 1"):
        v.decode_ogg([files[0], bad])
