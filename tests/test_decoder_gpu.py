"""Decoder on the MI355X: device unpack = host unpack bit for bit, spectrum exact against a float32 restatement of the
oracle's captures, PCM within a bound of a float64 IMDCT + window + overlap-add and bit for bit against the oracle's
scalar inverse MDCT + float32 window + overlap-add, the reference's own round-trip test (test/test.c), a full-size
batch, and the API edges."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

from tests import orc
from tests.signals import burst_signal, synth_signal
from tests.test_decoder_cpu import (DATA, ENOTAUDIO, PARITY, floor_expected, oracle_packets, pack_setup,
                                    residue_coded)
from tests.test_reference_input_gpu import classes, gen_windowed_sine
from tests.test_stream_wrapper import unpack_headers
import vpk  # noqa: E402  (tools/, on the path once test_stream_wrapper is imported)

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PACKS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DATA, "mode_*.vpk")))
EINVAL = -131


def rows_tensor(packets, dev, stride=None):
    stride = stride or max(1, max(len(p) for p in packets))
    a = np.zeros((len(packets), stride), np.uint8)
    for i, p in enumerate(packets):
        a[i, :len(p)] = np.frombuffer(p, np.uint8)
    nb = np.array([len(p) for p in packets], np.int32)
    return torch.from_numpy(a).to(dev), torch.from_numpy(nb).to(dev)


def split_dump(d):
    out, at = [], 0
    while at < len(d):
        n = int.from_bytes(d[at:at + 4], "little")
        out.append(d[at + 4:at + 4 + n])
        at += 4 + n
    return out


def pack_oracle_packets(oracle, pack, seconds=2.0):
    d = vpk.read_vpk(os.path.join(DATA, pack))
    ch, rate, q = int(d["info/channels"][0]), int(d["info/rate"][0]), float(d["info/quality"][0])
    bitrate = None
    if int(d["info/managed"][0]):
        av, mn, mx, _ = [int(x) for x in d["bi/rates"]]
        bitrate = (mx, av, mn)
    st = orc.Stream(orc.Setup(oracle, ch, rate, None if bitrate else q, bitrate=bitrate))
    oracle.lib.orc_stream_set_capture(st.v, 0)
    sig = burst_signal(ch, rate, int(seconds * rate), seed=11)
    out = []
    for i in range(0, sig.shape[1], 1024):
        st.write(sig[:, i:i + 1024])
        out += [b["packet"] for b in st.blocks()]
    st.finish()
    out += [b["packet"] for b in st.blocks()]
    st.close()
    return out


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
@pytest.mark.parametrize("ch,rate,q,golden", [
    (2, 44100, 0.5, "ref_scalar_2ch_44100_q05_20s.pkt"),
    (6, 48000, 0.8, "ref_scalar_6ch_48000_q08_10s.pkt"),
])
def test_device_unpack_of_the_reference_dumps(oracle, cuda, ch, rate, q, golden):
    import vorbis_aotuv_lancer_amd as v
    ds = v.DecodeSetup(v.header_packets(v.Setup(ch, rate, q)))
    packets = split_dump(open(os.path.join(G, golden), "rb").read())
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


@functools.lru_cache(maxsize=None)
def _cosines(N):
    k, t = np.arange(N // 2), np.arange(N)
    return np.cos(2 * np.pi / N * np.outer(t + 0.5 + N / 4, k + 0.5))


def imdct64(X):
    """float64 mdct_backward: C^T X with C[k, n] = cos(2 pi / N (n + 1/2 + N/4)(k + 1/2)) (the reference's forward is
    4/N C x; window, forward, backward, window and overlap-add return the input)"""
    return _cosines(2 * len(X)) @ X.astype(np.float64)


def overlap64(tail, lW, p, W, bs, win):
    """vorbis_synthesis_blockin's overlap-add in float64: what becomes final, and the new tail"""
    n0, n1 = bs[0] // 2, bs[1] // 2
    w0, w1 = win[0].astype(np.float64), win[1].astype(np.float64)
    n = bs[W] // 2
    if lW < 0:
        return np.zeros(0), p[n:2 * n].copy()
    if lW == 1 and W == 1:
        out = tail[:n1] * w1[::-1] + p[:n1] * w1
    elif lW == 1:
        off = n1 // 2 - n0 // 2
        out = np.concatenate([tail[:off], tail[off:off + n0] * w0[::-1] + p[:n0] * w0])
    elif W == 1:
        off = n1 // 2 - n0 // 2
        out = np.concatenate([tail[:n0] * w0[::-1] + p[off:off + n0] * w0, p[off + n0:off + n0 + off]])
    else:
        out = tail[:n0] * w0[::-1] + p[:n0] * w0
    return out, p[n:2 * n].copy()


def check_pcm_bound(ds, streams_pk, pcm_steps, spec_steps, info_steps, samples_steps, win=None, peaks=None):
    """per stream: the device PCM of every step against float64 IMDCT + window + OLA of the fetched spectrum.
    win: the two windows' rising halves (default: the product's own table); peaks: a list that receives every step's
    float64 peak"""
    import vorbis_aotuv_lancer_amd as v
    bs = ds.blocksizes
    if win is None:
        win = [v.window_table(bs[0]), v.window_table(bs[1])]
    worst = 0.0
    for s in range(len(streams_pk)):
        tail, lW = None, -1
        for t in range(len(streams_pk[s])):
            W = int(info_steps[t][s][1])
            n = bs[W] // 2
            p = np.stack([imdct64(spec_steps[t][s][c][:n]) for c in range(ds.channels)])
            outs, tails = [], []
            for c in range(ds.channels):
                o, tl = overlap64(tail[c] if tail is not None else None, lW, p[c], W, bs, win)
                outs.append(o)
                tails.append(tl)
            tail, lW = tails, W
            want = np.stack(outs)
            ns = int(samples_steps[t][s])
            # the end-of-stream packet is trimmed to its granule position (lib/block.c:1084-1161): the first ns stay
            last = t == len(streams_pk[s]) - 1
            assert ns == want.shape[1] or (last and ns < want.shape[1]), (s, t, ns, want.shape[1])
            want = want[:, :ns]
            got = pcm_steps[t][s][:, :ns].astype(np.float64)
            if ns:
                if peaks is not None:
                    peaks.append(float(np.abs(want).max()))
                peak = max(np.abs(want).max(), 1e-3)
                err = np.abs(got - want).max()
                worst = max(worst, err / peak)
                assert err <= 1e-5 * peak, f"stream {s} step {t}: max error {err} at peak {peak}"
    return worst


def overlap32(tail, lW, p, W, n0, n1, w0, w1):
    """overlap64 in float32: numpy rounds each product and the sum separately, as vorbis_synthesis_blockin's scalar
    pcm[i]*w[n-i-1] + p[i]*w[i] does with contraction off.  n0 / n1: half the two block sizes (a quarter at half
    rate), w0 / w1 the rising half windows of those lengths"""
    n = n1 if W else n0
    if lW < 0:
        return np.zeros(0, np.float32), p[n:2 * n].copy()
    if lW == 1 and W == 1:
        out = tail[:n1] * w1[::-1] + p[:n1] * w1
    elif lW == 1:
        off = n1 // 2 - n0 // 2
        out = np.concatenate([tail[:off], tail[off:off + n0] * w0[::-1] + p[:n0] * w0])
    elif W == 1:
        off = n1 // 2 - n0 // 2
        out = np.concatenate([tail[:n0] * w0[::-1] + p[off:off + n0] * w0, p[off + n0:off + n0 + off]])
    else:
        out = tail[:n0] * w0[::-1] + p[:n0] * w0
    assert out.dtype == np.float32
    return out, p[n:2 * n].copy()


def ulps_apart(a, b):
    """distance of two float32 values in representable values (-0.0 and 0.0 are 0 apart)"""
    def key(x):
        i = int(np.array(x, np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))


def check_pcm_exact(oracle, ds, streams_pk, pcm_steps, spec_steps, info_steps, samples_steps, halfrate=False):
    """check_pcm_bound's walk with a float32 yardstick and no tolerance: the device PCM of every step, stream and
    channel equals (np.array_equal) the oracle's scalar inverse MDCT (oracle/orc_mdct.c: orc_mdct_backward, itself
    checked against the float64 definition in tests/test_oracle_mdct.py) of the float32 spectrum, overlap-added in
    float32 with the product's own window tables, the tail carried in float32.  At half rate the transform has half the
    block's points over the lower half of the bins, and the windows are those of half the size.
    -> the number of (step, stream) pairs compared"""
    import vorbis_aotuv_lancer_amd as v
    bs = ds.blocksizes
    hs = 1 if halfrate else 0
    n0, n1 = bs[0] >> (1 + hs), bs[1] >> (1 + hs)
    w0, w1 = v.window_table(bs[0] >> hs), v.window_table(bs[1] >> hs)
    assert w0.dtype == np.float32 and w1.dtype == np.float32 and (len(w0), len(w1)) == (n0, n1)
    compared = 0
    for s in range(len(streams_pk)):
        tail, lW = None, -1
        for t in range(len(streams_pk[s])):
            W = int(info_steps[t][s][1])
            N = bs[W] >> hs                                            # points of the transform
            spec = np.stack([np.asarray(spec_steps[t][s][c][:N // 2], np.float32) for c in range(ds.channels)])
            p = oracle.mdct_backward(spec)
            outs, tails = [], []
            for c in range(ds.channels):
                o, tl = overlap32(tail[c] if tail is not None else None, lW, p[c], W, n0, n1, w0, w1)
                outs.append(o)
                tails.append(tl)
            tail, lW = tails, W
            want = np.stack(outs)
            ns = int(samples_steps[t][s])
            last = t == len(streams_pk[s]) - 1
            assert ns == want.shape[1] or (last and ns < want.shape[1]), (s, t, ns, want.shape[1])
            want = want[:, :ns]
            got = pcm_steps[t][s][:, :ns]
            assert got.dtype == np.float32 and want.dtype == np.float32
            if not np.array_equal(got, want):
                c, i = (int(x[0]) for x in np.nonzero(got != want))
                raise AssertionError(
                    f"stream {s} step {t} channel {c} sample {i} (block of {bs[W]}, after {'none' if lW < 0 else bs[lW]}"
                    f"{', half rate' if hs else ''}): device {float(got[c, i]):.9g}, scalar inverse MDCT {float(want[c, i]):.9g}, "
                    f"{ulps_apart(got[c, i], want[c, i])} ulps apart; {int((got != want).sum())} of {got.size} differ")
            compared += 1 if ns else 0
    return compared


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


def device_encode(v, setup, sig, cuda, S=1):
    """device front end, end of stream declared: -> per stream [(packet, granulepos, eos)]"""
    enc = v.Encoder(setup, S)
    fe = v.FrontEnd(enc)
    fe.write(torch.from_numpy(np.repeat(sig[None], S, axis=0)).to(cuda))
    fe.finish()
    got = [[] for _ in range(S)]
    while True:
        info, packets, nbytes = fe.encode_round()
        if len(info) == 0:
            break
        packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
        for k, pi in enumerate(info):
            got[int(pi["stream"])].append((bytes(packets[k, :nbytes[k]]), int(pi["granulepos"]), int(pi["eos"])))
    fe.close()
    enc.close()
    return got


def decode_one(v, ds, packets, cuda):
    """one stream, one packet per call, with granulepos and eos -> decoded PCM [ch, n]"""
    dec = v.Decoder(ds, 1, 1)
    out = []
    for p, gp, eos in packets:
        pk, nb = rows_tensor([p], cuda)
        pcm, samples, status = dec.synthesis_batch(
            [0], pk, nb, granulepos=torch.tensor([gp], dtype=torch.int64, device=cuda),
            eos=torch.tensor([eos], dtype=torch.uint8, device=cuda))
        assert int(status[0]) == 0
        out.append(pcm[0, :, :int(samples[0])].cpu().numpy())
    dec.close()
    return np.concatenate(out, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("ch,rate,q,bitrate", [c + (None,) for c in classes()] + [(2, 44100, None, 128000),
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
