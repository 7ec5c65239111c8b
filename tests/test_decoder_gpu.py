"""Decoder on the MI355X: device unpack = host unpack bit for bit, spectrum exact against a float32 restatement of the
oracle's captures, PCM within a bound of a float64 IMDCT + window + overlap-add and bit for bit against the oracle's
scalar inverse MDCT + float32 window + overlap-add, the reference's own round-trip test (test/test.c), a full-size
batch, and the API edges."""
import os

import numpy as np
import pytest
import torch

from tests import orc
from tests.decode_calls import check_pcm_bound, check_pcm_exact, decode_one, device_encode, rows_tensor
from tests.decode_packets import (DATA, DUMPS, EINVAL, ENOTAUDIO, PACKS, PARITY, dump_packets, floor_expected,
                                  matrix_classes, oracle_packets, pack_setup, residue_coded, unpack_headers, vpk)
from tests.signals import gen_windowed_sine, synth_signal


def pack_oracle_packets(oracle, pack, seconds=2.0):
    d = vpk.read_vpk(os.path.join(DATA, pack))
    ch, rate, q = int(d["info/channels"][0]), int(d["info/rate"][0]), float(d["info/quality"][0])
    bitrate = None
    if int(d["info/managed"][0]):
        av, mn, mx, _ = [int(x) for x in d["bi/rates"]]
        bitrate = (mx, av, mn)
    return [b["packet"] for b in oracle_packets(oracle, ch, rate, q, seconds, seed=11, bitrate=bitrate, capture=False)]


def device_vs_host(ds, dec, packets, dev):
    """one call with one packet per (fresh) stream; every intermediate equals the host unpack"""
    ids = list(range(len(packets)))
    pk, nb = rows_tensor(packets, dev)
    pcm, samples, status = dec.synthesis_batch(ids, pk, nb)
    got = {n: dec.fetch(n).cpu().numpy() for n in ("info", "floor_index", "floor_used", "residue")}
    status, samples = status.cpu().numpy(), samples.cpu().numpy()
    for k, p in enumerate(packets):
        rc, info, findex, res, used = ds.unpack(p)
        assert status[k] == rc, f"row {k}"
        assert samples[k] == 0                          # first packet of every stream
        if rc:
            continue
        assert list(got["info"][k]) == info, f"row {k}"
        np.testing.assert_array_equal(got["floor_index"][k], findex, err_msg=f"row {k}: floor index")
        np.testing.assert_array_equal(got["floor_used"][k], used, err_msg=f"row {k}: floor used")
        assert got["residue"][k].tobytes() == res.tobytes(), f"row {k}: residue"


@pytest.mark.gpu
@pytest.mark.parametrize("pack", PACKS)
def test_device_unpack_equals_host_unpack(oracle, cuda, pack):
    import vorbis_aotuv_lancer_amd as v
    setup, d = pack_setup(v, pack)
    ds = v.DecodeSetup(v.header_packets(setup))
    packets = pack_oracle_packets(oracle, pack)
    # truncated packets: a long and a short one at every length, and every packet cut in half
    longp = max(packets, key=len)
    shortp = min(packets[1:], key=len)
    cuts = [longp[:n] for n in range(0, len(longp), max(1, len(longp) // 97))] + [shortp[:n] for n in range(len(shortp))]
    cuts += [p[:len(p) // 2] for p in packets]
    rows = packets + cuts + v.header_packets(setup)
    dec = v.Decoder(ds, len(rows), len(rows))
    device_vs_host(ds, dec, rows, cuda)
    dec.close()
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ch,rate,q,golden", DUMPS)
def test_device_unpack_of_the_reference_dumps(oracle, cuda, ch, rate, q, golden):
    import vorbis_aotuv_lancer_amd as v
    ds = v.DecodeSetup(v.header_packets(v.Setup(ch, rate, q)))
    packets = dump_packets(golden)
    dec = v.Decoder(ds, len(packets), len(packets))
    device_vs_host(ds, dec, packets, cuda)
    dec.close()
    # the first 200 packets as four streams of 50 consecutive ones, decoded stepwise: PCM bounded and exact
    S, T = 4, 50
    dec = v.Decoder(ds, S, S)
    pcm_steps, spec_steps, info_steps, samples_steps = [], [], [], []
    for t in range(T):
        pk, nb = rows_tensor([packets[s * T + t] for s in range(S)], cuda)
        pcm, samples, status = dec.synthesis_batch(list(range(S)), pk, nb)
        assert not status.cpu().numpy().any()
        pcm_steps.append(pcm.cpu().numpy())
        spec_steps.append(dec.fetch("spectrum").cpu().numpy())
        info_steps.append(dec.fetch("info").cpu().numpy())
        samples_steps.append(samples.cpu().numpy())
    assert {int(i[1]) for step in info_steps for i in step} == {0, 1}      # both block sizes
    streams = [list(range(T))] * S
    worst = check_pcm_bound(ds, streams, pcm_steps, spec_steps, info_steps, samples_steps)
    exact = check_pcm_exact(oracle, ds, streams, pcm_steps, spec_steps, info_steps, samples_steps)
    print(f"\n{golden}: max |pcm - float64 reference| / peak = {worst:.3g}; {exact} steps x streams equal the scalar "
          f"inverse MDCT bit for bit")
    dec.close()
    ds.close()


def restated_spectrum(ref, fromdB, enc_x1, b, mode, n):
    """numpy float32: inverse square-polar coupling of the residue ints (reverse step order), then one multiply by
    FLOOR1_fromdB_LOOKUP[floor index]; 0 on channels whose floor is not coded (floor1_inverse2)"""
    ch = b["residue"].shape[0]
    mask = residue_coded(ref, mode, ch, n, b["nonzero"])
    v = np.where(mask, b["residue"].astype(np.float32), np.float32(0))
    m = ref["maps"][ref["modes"][mode][3]]
    for mag, ang in reversed(m["coupling"]):
        M, A = v[mag].copy(), v[ang].copy()
        pm = np.where(M > 0, np.where(A > 0, M, M + A), np.where(A > 0, M, M - A))
        pa = np.where(M > 0, np.where(A > 0, M - A, M), np.where(A > 0, M + A, M))
        v[mag], v[ang] = pm.astype(np.float32), pa.astype(np.float32)
    findex = floor_expected(ref, enc_x1, mode, b["ilogmask"], n)
    out = v * fromdB[findex]
    out[np.asarray(b["post_valid"]) == 0] = 0
    return out.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("ch,rate,q", PARITY)
def test_spectrum_exact_and_pcm_bounded(oracle, cuda, ch, rate, q):
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(ch, rate, q))
    ref = unpack_headers(*h)
    ds = v.DecodeSetup(h)
    fromdB = v.tables.pack("common.vpk")["FLOOR1_fromdB_LOOKUP"]
    pack = vpk.read_vpk(os.path.join(DATA, orc.mode_pack_name(ch, rate, q)))
    enc_x1 = [int(pack[f"floor/{i}/postlist"][1]) for i in range(len(ref["floors"]))]
    S = 3
    blocks = [oracle_packets(oracle, ch, rate, q, seconds=2.0, seed=20 + s) for s in range(S)]
    steps = min(len(b) for b in blocks)
    dec = v.Decoder(ds, S, S)
    pcm_steps, spec_steps, info_steps, samples_steps = [], [], [], []
    for t in range(steps):
        pk, nb = rows_tensor([blocks[s][t]["packet"] for s in range(S)], cuda)
        pcm, samples, status = dec.synthesis_batch(list(range(S)), pk, nb)
        assert not status.cpu().numpy().any()
        spec = dec.fetch("spectrum").cpu().numpy()
        info = dec.fetch("info").cpu().numpy()
        for s in range(S):
            b, mode, W = blocks[s][t], int(info[s][0]), int(info[s][1])
            n = ds.blocksizes[W] // 2
            want = restated_spectrum(ref, fromdB, enc_x1, b, mode, n)
            assert spec[s][:, :n].tobytes() == want.tobytes(), f"stream {s} packet {t}: spectrum"
            assert not spec[s][:, n:].any()
        pcm_steps.append(pcm.cpu().numpy())
        spec_steps.append(spec)
        info_steps.append(info)
        samples_steps.append(samples.cpu().numpy())
    worst = check_pcm_bound(ds, [list(range(steps))] * S, pcm_steps, spec_steps, info_steps, samples_steps)
    print(f"\n{ch}ch {rate} q{q}: max |pcm - float64 reference| / peak = {worst:.3g}")
    exact = check_pcm_exact(oracle, ds, [list(range(steps))] * S, pcm_steps, spec_steps, info_steps, samples_steps)
    print(f"{ch}ch {rate} q{q}: {exact} steps x streams equal the scalar inverse MDCT bit for bit")
    dec.close()
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ch,rate,q,bitrate", [c + (None,) for c in matrix_classes()] + [(2, 44100, None, 128000),
                                                                                   (6, 48000, 0.8, None)])
def test_reference_round_trip(cuda, ch, rate, q, bitrate):
    """test/test.c: the windowed sine of test/util.c, encoded with end of stream, decodes to exactly its 2048 samples
    with a peak within 0.95 +- (0.15 - 0.1 q)"""
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(ch, rate, bitrate=bitrate) if bitrate else v.Setup(ch, rate, q)
    sine = gen_windowed_sine()
    pcm = np.repeat(sine[None, :], ch, axis=0)
    packets = device_encode(v, setup, pcm, cuda)[0]
    assert packets[-1][2] == 1 and packets[-1][1] == 2048
    ds = v.DecodeSetup(v.header_packets(setup))
    out = decode_one(v, ds, packets, cuda)
    assert out.shape == (ch, 2048)
    qq = q if q is not None else 0.5
    allowable = 0.15 - 0.1 * qq
    peak = float(np.abs(out).max())
    assert 0.95 - allowable <= peak <= 0.95 + allowable, peak
    ds.close()


@pytest.mark.gpu
def test_full_size_twins_unsynchronised_steps(oracle, cuda):
    """16384 stereo q0.5 streams of ~2 s, K signals dealt round robin, decoded in steps that never wait for the host:
    every stream decodes to its twin's PCM, and the K leads pass the unpack and PCM checks"""
    import vorbis_aotuv_lancer_amd as v
    S, K, ch, rate, q = 16384, 8, 2, 44100, 0.5
    nchunks = 86                                           # 86 * 1024 samples ~ 2 s
    sigs = [synth_signal(ch, rate, nchunks * 1024, seed=700 + k, level=1.0 if k % 3 else 0.05) for k in range(K)]
    setup = v.Setup(ch, rate, q)
    enc = v.Encoder(setup, S)
    fe = v.FrontEnd(enc)
    base = torch.from_numpy(np.stack(sigs)).to(cuda)
    lead = [[] for _ in range(K)]                          # (packetno, packet, granulepos, eos) of stream k < K
    row_of = np.full(S, -1, np.int64)

    def take(info, packets, nbytes):
        packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
        st = info["stream"].astype(np.int64)
        row_of[:] = -1
        row_of[st] = np.arange(len(st))
        lr = row_of[st % K]
        assert (lr >= 0).all()
        w = int(nbytes.max())
        pk = packets[:, :w]
        cols = np.arange(w)[None, :]
        same = ((pk == pk[lr]) | (cols >= nbytes[:, None])).all(axis=1) & (nbytes == nbytes[lr])
        assert same.all(), "a stream's packet differs from its twin's"
        for r in np.nonzero(st < K)[0]:
            lead[st[r]].append((int(info["packetno"][r]), bytes(packets[r, :nbytes[r]]), int(info["granulepos"][r]),
                                int(info["eos"][r])))

    for c in range(nchunks):
        fe.write(base[:, :, c * 1024:(c + 1) * 1024].repeat(S // K, 1, 1).contiguous())
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                break
            take(info, packets, nbytes)
    fe.finish()
    while True:
        info, packets, nbytes = fe.encode_round()
        if len(info) == 0:
            break
        take(info, packets, nbytes)
    fe.close()
    enc.close()
    for k in range(K):
        lead[k].sort()
        assert [p[0] for p in lead[k]] == list(range(3, 3 + len(lead[k])))
    steps = max(len(x) for x in lead)
    stride = max(len(p[1]) for x in lead for p in x)
    # device-resident inputs of every step: lead packets [K, steps, stride]; a stream reads its lead's row
    lp = np.zeros((K, steps, stride), np.uint8)
    lnb = np.zeros((K, steps), np.int32)
    lgp = np.full((K, steps), -1, np.int64)
    leos = np.zeros((K, steps), np.uint8)
    for k in range(K):
        for t, (_, p, gp, e) in enumerate(lead[k]):
            lp[k, t, :len(p)] = np.frombuffer(p, np.uint8)
            lnb[k, t], lgp[k, t], leos[k, t] = len(p), gp, e
    lp, lnb, lgp, leos = (torch.from_numpy(a).to(cuda) for a in (lp, lnb, lgp, leos))
    ds = v.DecodeSetup(v.header_packets(setup))
    dec = v.Decoder(ds, S, S)
    mism = torch.zeros((), dtype=torch.int64, device=cuda)
    keep = []
    ids_all = np.arange(S)
    for t in range(steps):
        alive = np.array([t < len(lead[k]) for k in range(K)])
        ids = ids_all[alive[ids_all % K]]
        li = torch.from_numpy(ids % K).to(cuda)           # host -> device copy only; nothing waits for the device
        pk = lp[li, t].contiguous()
        out = (torch.zeros((len(ids), ch, ds.blocksizes[1] // 2), dtype=torch.float32, device=cuda),
               torch.empty(len(ids), dtype=torch.int32, device=cuda), torch.empty(len(ids), dtype=torch.int32, device=cuda))
        pcm, samples, status = dec.synthesis_batch(ids, pk, lnb[li, t], granulepos=lgp[li, t], eos=leos[li, t], out=out)
        # twins: row r equals the row of its lead (the first K rows of every step are the leads, ids sorted)
        nl = int(alive.sum())
        lead_row = torch.from_numpy(np.searchsorted(ids, ids % K)).to(cuda)
        mism += (pcm != pcm[lead_row]).flatten(1).any(dim=1).sum() + (samples != samples[lead_row]).sum()
        mism += (status != 0).sum()
        fetched = {n: dec.fetch(n)[:nl].clone() for n in ("info", "floor_index", "floor_used", "residue", "spectrum")}
        keep.append((ids[:nl] % K, pcm[:nl].clone(), samples[:nl].clone(), fetched))
    torch.cuda.synchronize()
    assert int(mism) == 0
    total = np.zeros(K, np.int64)
    pcm_steps, spec_steps, info_steps, samples_steps = [], [], [], []
    for t, (lk, pcm, samples, f) in enumerate(keep):
        pcm, samples = pcm.cpu().numpy(), samples.cpu().numpy()
        fn = {n: x.cpu().numpy() for n, x in f.items()}
        for j, k in enumerate(lk):
            rc, info, findex, res, used = ds.unpack(lead[k][t][1])
            assert rc == 0 and list(fn["info"][j]) == info
            assert np.array_equal(fn["floor_index"][j], findex) and np.array_equal(fn["floor_used"][j], used)
            assert fn["residue"][j].tobytes() == res.tobytes()
            total[k] += samples[j]
        full = np.zeros((K,) + pcm.shape[1:], np.float32)
        fs = np.zeros((K,) + fn["spectrum"].shape[1:], np.float32)
        fi = np.zeros((K, 4), np.int32)
        sm = np.zeros(K, np.int32)
        full[lk], fs[lk], fi[lk], sm[lk] = pcm, fn["spectrum"], fn["info"], samples
        pcm_steps.append(full)
        spec_steps.append(fs)
        info_steps.append(fi)
        samples_steps.append(sm)
    # the decoded length of every stream is what was written
    assert (total == nchunks * 1024).all(), total
    worst = check_pcm_bound(ds, [lead[k] for k in range(K)], pcm_steps, spec_steps, info_steps, samples_steps)
    print(f"\nfull size: max |pcm - float64 reference| / peak = {worst:.3g}")
    exact = check_pcm_exact(oracle, ds, [lead[k] for k in range(K)], pcm_steps, spec_steps, info_steps, samples_steps)
    print(f"full size: {exact} steps x streams equal the scalar inverse MDCT bit for bit")
    dec.close()
    ds.close()


@pytest.mark.gpu
def test_edges_duplicates_header_as_audio_restart(oracle, cuda):
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(2, 44100, 0.5))
    ds = v.DecodeSetup(h)
    blocks = oracle_packets(oracle, 2, 44100, 0.5, seconds=1.0)
    pk = [b["packet"] for b in blocks]
    dec = v.Decoder(ds, 4, 4)
    rows, nb = rows_tensor(pk[:2], cuda)
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        dec.synthesis_batch([1, 1], rows, nb)
    # stream 0: the packets; stream 1: the same with a header packet in between (skipped, state untouched)
    outs = {0: [], 1: []}
    for t in range(6):
        if t == 3:
            r, n = rows_tensor([h[2]], cuda)
            pcm, samples, status = dec.synthesis_batch([1], r, n)
            assert int(status[0]) == ENOTAUDIO and int(samples[0]) == 0
        r, n = rows_tensor([pk[t], pk[t]], cuda)
        pcm, samples, status = dec.synthesis_batch([0, 1], r, n)
        assert not status.cpu().numpy().any()
        s = samples.cpu().numpy()
        assert s[0] == s[1] and (t > 0 or s[0] == 0)
        outs[0].append(pcm[0, :, :s[0]].cpu().numpy())
        outs[1].append(pcm[1, :, :s[1]].cpu().numpy())
    assert np.array_equal(np.concatenate(outs[0], 1), np.concatenate(outs[1], 1))
    # restart: the next packet returns nothing
    dec.restart_streams([0])
    r, n = rows_tensor([pk[6], pk[6]], cuda)
    pcm, samples, status = dec.synthesis_batch([0, 1], r, n)
    s = samples.cpu().numpy()
    assert s[0] == 0 and s[1] > 0
    dec.reset()
    pcm, samples, status = dec.synthesis_batch([0, 1], r, n)
    assert not samples.cpu().numpy().any()
    dec.close()
    ds.close()
