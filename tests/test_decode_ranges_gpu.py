"""Seekable range decoding on the MI355X (RangeStore, Decoder.synthesis_ranges, OggIndex): every window is bit for bit
(np.array_equal on float32) the same slice of the stream's linear decode, which is the stepwise decode (one packet
per stream per call through synthesis_batch) or decode_ogg."""
import ctypes

import numpy as np
import pytest
import torch

from tests.decode_calls import (FILL_RANGES, check, device_encode, encode_chunked, encoded, linear, ranges,
                                rows_tensor, runs_call, stepwise)
from tests.decode_packets import EINVAL, ENOTAUDIO, as_stream, pack_setup
from tests.signals import burst_signal, gen_windowed_sine, synth_signal


CLASSES = ["mode_1ch_44100_q0.5.vpk", "mode_2ch_44100_q0.5.vpk", "mode_6ch_48000_q0.5.vpk", "mode_1ch_8000_q0.5.vpk",
           "mode_2ch_96000_q0.5.vpk"]


@pytest.mark.gpu
@pytest.mark.parametrize("pack", CLASSES)
def test_index_and_ranges_per_class(cuda, pack):
    import vorbis_aotuv_lancer_amd as v
    setup, _ = pack_setup(v, pack)
    pks = [encoded(v, setup, 2.0, 81, cuda, burst=True), encoded(v, setup, 1.3, 82, cuda)]
    ds = v.DecodeSetup(v.header_packets(setup))
    if pack == "mode_1ch_8000_q0.5.vpk":
        assert ds.blocksizes == (512, 512)
    want = stepwise(v, ds, pks, cuda)
    lin = [w[0] for w in want]
    for pk, w in zip(pks, want):
        st = as_stream(pk)
        status, samples, out_start, total = v.decode_index(ds, *st)
        assert list(status) == w[2] and list(samples) == w[1] and total == w[0].shape[1]
    dec = v.Decoder(ds, 1, 64)
    store = v.RangeStore(dec, [as_stream(pk) for pk in pks])
    assert list(store.totals) == [x.shape[1] for x in lin]
    rng = np.random.default_rng(5)
    ids = [int(i) for i in rng.integers(0, 2, 40)]
    starts = [int(rng.integers(0, lin[i].shape[1] + 10)) for i in ids]
    lengths = [int(rng.integers(0, 9000)) for _ in ids]
    pcm, got = ranges(dec, store, ids, starts, lengths)
    check(lin, ids, starts, lengths, pcm, got, pack)
    store.close()
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_random_ranges_of_files_equal_decode_ogg(cuda, tmp_path):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    files = []
    for i in range(5):
        pk = encoded(v, setup, 1.0 + 0.7 * i, 90 + i, cuda, burst=i % 2 == 1)
        blob = v.write_ogg(setup, [p[0] for p in pk], [(p[1], p[2]) for p in pk], serialno=i)
        if i == 2:
            path = tmp_path / "two.ogg"
            path.write_bytes(blob)
            blob = str(path)
        files.append(blob)
    lin = [p.cpu().numpy() for p, _ in v.decode_ogg(files)]
    idx = v.OggIndex(files, max_batch=256)
    assert list(idx.total_samples) == [x.shape[1] for x in lin]
    rng = np.random.default_rng(11)
    ids = [int(i) for i in rng.integers(0, 5, 300)]
    starts = [int(rng.integers(0, lin[i].shape[1])) for i in ids]
    lengths = [int(rng.integers(1, 44100)) for _ in ids]
    pcm, got = idx.decode_ranges(ids, starts, lengths)
    assert pcm.is_cuda and pcm.dtype == torch.float32 and tuple(pcm.shape) == (300, 2, max(lengths))
    pcm = pcm.cpu().numpy()
    for r, (i, s, L) in enumerate(zip(ids, starts, lengths)):
        n = min(lin[i].shape[1] - s, L)
        assert got[r] == n and np.array_equal(pcm[r, :, :n], lin[i][:, s:s + n]) and np.all(pcm[r, :, n:] == 0)
    idx.close()
    mono = v.Setup(1, 44100, 0.5)
    pk = encoded(v, mono, 0.5, 99, cuda)
    other = v.write_ogg(mono, [p[0] for p in pk], [(p[1], p[2]) for p in pk], serialno=9)
    with pytest.raises(ValueError):
        v.OggIndex([files[0], other])


@pytest.mark.gpu
def test_edge_cases_and_overlapping_ranges(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    pk = encoded(v, setup, 3.0, 95, cuda, burst=True)
    ds = v.DecodeSetup(v.header_packets(setup))
    lin = [linear(v, ds, pk, cuda)]
    total = lin[0].shape[1]
    _, samples, out_start, _ = v.decode_index(ds, *as_stream(pk))
    dec = v.Decoder(ds, 1, 128)
    store = v.RangeStore(dec, [as_stream(pk)])
    starts, lengths = [0, 0, 5, total - 1, total - 100, total - 100, total, total + 50, 0], \
                      [1, 3000, 0, 1, 100, 5000, 10, 10, total]
    for k in range(3, len(pk), 9):                        # packet starts and +-1
        if samples[k]:
            for d in (-1, 0, 1):
                starts.append(int(out_start[k]) + d)
                lengths.append([1, 700, 2048][(k + d) % 3])
    rng = np.random.default_rng(2)
    for _ in range(60):                                    # many overlapping ranges of one stream
        s = int(rng.integers(0, 20000))
        starts.append(s)
        lengths.append(int(rng.integers(1, 6000)))
    ids = [0] * len(starts)
    pcm, got = ranges(dec, store, ids, starts, lengths)
    check(lin, ids, starts, lengths, pcm, got, "edges")
    assert got[2] == 0 and got[6] == 0 and got[7] == 0 and got[5] == 100 and got[8] == total
    pcm, got = ranges(dec, store, [], [], [])
    assert len(got) == 0
    store.close()
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_runs_constructions_trimmed_start_windowed_sine_failed_packets(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    h = v.header_packets(setup)
    pk = encoded(v, setup, 2.0, 44, cuda)
    low = [(p, -1, e) for p, _, e in pk[:4]] + list(pk[4:])
    low[4] = (low[4][0], low[4][1] - 700, low[4][2])
    rng = np.random.default_rng(1)
    bad = list(pk)
    bad.insert(10, (h[2], -1, 0))
    bad.insert(20, (pk[19][0][:len(pk[19][0]) // 3], -1, 0))
    bad.insert(30, (rng.integers(0, 256, 200, dtype=np.uint8).tobytes(), -1, 0))
    for _ in range(12):                                   # a pre-roll behind many failed packets
        bad.insert(41, (b"", -1, 0))
    bad.insert(0, (h[0], -1, 0))
    sine = device_encode(v, setup, np.repeat(gen_windowed_sine()[None, :], 2, axis=0), cuda)[0]
    streams = [low, bad, sine]
    ds = v.DecodeSetup(h)
    lin = [w[0] for w in stepwise(v, ds, streams, cuda)]
    assert lin[2].shape == (2, 2048)
    st_bad = v.decode_index(ds, *as_stream(bad))
    assert st_bad[0][0] == ENOTAUDIO and sum(1 for s in st_bad[0] if s) >= 14
    for mb in (64, 7, 2):
        dec = v.Decoder(ds, 1, mb)
        store = v.RangeStore(dec, [as_stream(s) for s in streams])
        ids, starts, lengths = [], [], []
        for i, x in enumerate(lin):
            for s in list(range(0, x.shape[1], 997)) + [0, x.shape[1] - 1]:
                ids.append(i)
                starts.append(s)
                lengths.append(3001)
        ids += [1, 1, 0]
        starts += [int(st_bad[2][41]) - 5, int(st_bad[2][53]) - 1, 0]
        lengths += [4000, 2500, lin[0].shape[1]]
        pcm, got = ranges(dec, store, ids, starts, lengths)
        check(lin, ids, starts, lengths, pcm, got, f"max_batch {mb}")
        store.close()
        dec.close()
    ds.close()


@pytest.mark.gpu
def test_pieces_and_sub_calls_give_the_same_bits(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    pks = [encoded(v, setup, 4.0, 120 + k, cuda, burst=k == 1) for k in range(3)]
    ds = v.DecodeSetup(v.header_packets(setup))
    rng = np.random.default_rng(8)
    ids = [int(i) for i in rng.integers(0, 3, 50)]
    starts = [int(rng.integers(0, 150000)) for _ in ids]
    lengths = [int(rng.integers(1, 60000)) for _ in ids]
    outs = []
    for mb in (4096, 64, 7, 2):
        dec = v.Decoder(ds, 1, mb)
        store = v.RangeStore(dec, [as_stream(pk) for pk in pks])
        outs.append(ranges(dec, store, ids, starts, lengths))
        store.close()
        dec.close()
    lin = [linear(v, ds, pk, cuda) for pk in pks]
    check(lin, ids, starts, lengths, *outs[0], "one call")
    for pcm, got in outs[1:]:
        assert np.array_equal(got, outs[0][1]) and np.array_equal(pcm, outs[0][0])
    ds.close()


@pytest.mark.gpu
def test_range_calls_leave_stream_state_alone(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    pk = encoded(v, setup, 2.0, 130, cuda)
    ds = v.DecodeSetup(v.header_packets(setup))
    lin = [linear(v, ds, pk, cuda)]
    dec = v.Decoder(ds, 2, 64)
    store = v.RangeStore(dec, [as_stream(pk)])
    parts, rparts = [], []
    for a in range(0, len(pk), 20):
        out = runs_call(dec, [1], [pk[a:a + 20]], cuda)
        parts.append(out[0][0, :, :int(out[1][0])].cpu().numpy())
        rparts.append(ranges(dec, store, [0, 0], [a * 300, 1000 + a], [2000, 17]))
        r, n = rows_tensor([pk[min(a, len(pk) - 1)][0]], cuda)
        dec.synthesis_batch([0], r, n)                   # stream 0 too, stepwise, between range calls
    assert np.array_equal(np.concatenate(parts, axis=1), lin[0])
    for k, (pcm, got) in enumerate(rparts):
        a = k * 20
        check(lin, [0, 0], [a * 300, 1000 + a], [2000, 17], pcm, got, f"interleaved {k}")
    store.close()
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_argument_errors_enqueue_nothing(cuda):
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    setup = v.Setup(2, 44100, 0.5)
    pk = encoded(v, setup, 1.0, 140, cuda)
    ds = v.DecodeSetup(v.header_packets(setup))
    lin = [linear(v, ds, pk, cuda)]
    dec = v.Decoder(ds, 1, 16)
    other = v.Decoder(ds, 1, 16)
    store = v.RangeStore(dec, [as_stream(pk)])
    out = torch.full((2, 2, 100), FILL_RANGES, device=cuda)
    for args in ([5], [0], [100]), ([0], [-1], [100]), ([0], [0], [-1]):
        with pytest.raises(v.VbmError, match=str(EINVAL)):
            dec.synthesis_ranges(store, *args)
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        dec.synthesis_ranges(store, [0, 0], [0, 10], [100, 101], out=out)        # pcm_stride 100 < 101
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        other.synthesis_ranges(store, [0], [0], [100])                          # a store of another decoder
    one = v.Decoder(ds, 1, 1)
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        one.synthesis_ranges(v.RangeStore(one, [as_stream(pk)]), [0], [0], [10])   # max_batch < 2
    torch.cuda.synchronize()
    assert torch.all(out == FILL_RANGES)
    ids, st, ln = np.array([0], np.int32), np.array([0], np.int64), np.array([10], np.int32)
    got = np.zeros(1, np.int32)
    assert lib.vbm_synthesis_ranges(dec._h, None, 1, ids.ctypes.data, st.ctypes.data, ln.ctypes.data,
                                    out.data_ptr(), 100, got.ctypes.data, None) == EINVAL
    bad_first = np.array([1, len(pk)], np.int64)                               # stream_packets[0] != 0
    data, offs, gp, eo = as_stream(pk)
    h = ctypes.c_void_p()
    assert lib.vbm_range_store_create(ctypes.byref(h), dec._h, 1, bad_first.ctypes.data, data.ctypes.data,
                                      offs.ctypes.data, len(data), gp.ctypes.data, eo.ctypes.data) == EINVAL
    pcm, got = ranges(dec, store, [0], [0], [1000])
    check(lin, [0], [0], [1000], pcm, got, "after the refused calls")
    store.close()
    dec.close()
    other.close()
    ds.close()


@pytest.mark.gpu
def test_full_size_ranges_unsynchronised(cuda):
    """thousands of 1 s ranges over hundreds of streams, calls back to back; a seeded subset checked bit for bit"""
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    K, S = 8, 256
    leads = [encode_chunked(v, setup, (burst_signal if k % 2 else synth_signal)(2, 44100, 6 * 44100 // 1024 * 1024,
                                                                               seed=400 + k), cuda) for k in range(K)]
    ds = v.DecodeSetup(v.header_packets(setup))
    lin = [linear(v, ds, pk, cuda) for pk in leads]
    dec = v.Decoder(ds, 1, 4096)
    store = v.RangeStore(dec, [as_stream(leads[s % K]) for s in range(S)])
    rng = np.random.default_rng(21)
    calls = []
    for c in range(4):
        ids = [int(i) for i in rng.integers(0, S, 2048)]
        starts = [int(rng.integers(0, store.totals[i])) for i in ids]
        out = torch.full((2048, 2, 44100), FILL_RANGES, dtype=torch.float32, device=cuda)
        pcm, got = dec.synthesis_ranges(store, ids, starts, [44100] * 2048, out=out)
        calls.append((ids, starts, pcm, got))
    torch.cuda.synchronize()
    for ids, starts, pcm, got in calls:
        pick = rng.choice(2048, 64, replace=False)
        sub = pcm[torch.from_numpy(pick).to(cuda)].cpu().numpy()
        check([lin[ids[r] % K] for r in pick], list(range(64)), [starts[r] for r in pick], [44100] * 64, sub,
              got[pick], "full size")
    store.close()
    dec.close()
    ds.close()
