"""Device-side driver of the decoder tests: the two builders that turn packet rows into the inputs of synthesis_batch
and synthesis_runs, the stepwise / runs / ranges calls built on them, the device encoder that makes real packets, and
the checks of decoded PCM (exact against the oracle's scalar inverse MDCT, bounded against float64).  The host-side
packet toolkit is tests/decode_packets.py."""
import functools

import numpy as np
import torch

from tests.signals import burst_signal, synth_signal

FILL_RANGES = 7.5        # what `ranges` puts where no range call writes
FILL_PLAYER = -77.25     # what the mixed players' output buffers hold before a call: no corpus stream's sample value


# ---- inputs ----------------------------------------------------------------------------------------------------------
def to_dev(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def rows_tensor(packets, dev):
    """[packet] -> synthesis_batch's (packets uint8 [rows, longest], nbytes int32 [rows]) on the device"""
    stride = max(1, max(len(p) for p in packets))
    a = np.zeros((len(packets), stride), np.uint8)
    for i, p in enumerate(packets):
        a[i, :len(p)] = np.frombuffer(p, np.uint8)
    nb = np.array([len(p) for p in packets], np.int32)
    return torch.from_numpy(a).to(dev), torch.from_numpy(nb).to(dev)


def batch_inputs(rows, dev):
    """rows [(packet, granulepos, eos)], one per stream -> synthesis_batch's (packets, nbytes, granulepos, eos)"""
    return (*rows_tensor([p[0] for p in rows], dev), to_dev(np.array([p[1] for p in rows], np.int64), dev),
            to_dev(np.array([p[2] for p in rows], np.uint8), dev))


def runs_inputs(runs, dev, marks=False):
    """runs: per run [(packet, granulepos, eos[, gap])], rows concatenated -> synthesis_runs' (data, offsets,
    granulepos, eos, gap) on the device.  gap is None where no row carries a mark, unless marks: then the tensor
    goes to the call even when it is all zero"""
    flat = [p for r in runs for p in r]
    data = np.frombuffer(b"".join(p[0] for p in flat) or b"\0", np.uint8).copy()
    offs = np.zeros(len(flat) + 1, np.int64)
    offs[1:] = np.cumsum([len(p[0]) for p in flat])
    gap = np.array([p[3] if len(p) > 3 else 0 for p in flat], np.uint8)
    return (to_dev(data, dev), to_dev(offs, dev), to_dev(np.array([p[1] for p in flat], np.int64), dev),
            to_dev(np.array([p[2] for p in flat], np.uint8), dev), to_dev(gap, dev) if marks or gap.any() else None)


# ---- calls -----------------------------------------------------------------------------------------------------------
def runs_call(dec, ids, runs, dev):
    """one synthesis_runs call -> device tensors (pcm, run_samples, samples, status)"""
    data, offs, gp, eo, gap = runs_inputs(runs, dev)
    return dec.synthesis_runs(ids, [len(r) for r in runs], data, offs, granulepos=gp, eos=eo, gap=gap)


def step_rows(dec, ids, rows, dev, pcm, samp, stat):
    """one synthesis_batch call, row r the next (packet, granulepos, eos) of stream ids[r], read back at once: every
    stream's PCM, samples and status go to the end of its lists pcm[s], samp[s], stat[s]"""
    pk, nb, gp, eo = batch_inputs(rows, dev)
    p, n, st = dec.synthesis_batch(ids, pk, nb, granulepos=gp, eos=eo)
    p, n, st = p.cpu().numpy(), n.cpu().numpy(), st.cpu().numpy()
    for r, s in enumerate(ids):
        pcm[s].append(p[r, :, :n[r]])
        samp[s].append(int(n[r]))
        stat[s].append(int(st[r]))


def stepwise(v, ds, streams, dev, restart_at=None, halfrate=False):
    """streams: per stream [(packet, granulepos, eos)], fed one packet per stream per call (synthesis_batch).
    restart_at: {stream: packet index} restarts the stream before that packet.
    -> per stream (pcm [ch, n], samples [P], status [P])"""
    S = len(streams)
    dec = v.Decoder(ds, S, S, halfrate=halfrate)
    pcm, samp, stat = [[] for _ in range(S)], [[] for _ in range(S)], [[] for _ in range(S)]
    for t in range(max(len(s) for s in streams)):
        ids = [s for s in range(S) if t < len(streams[s])]
        rs = [s for s in ids if restart_at and restart_at.get(s) == t]
        if rs:
            dec.restart_streams(rs)
        step_rows(dec, ids, [streams[s][t] for s in ids], dev, pcm, samp, stat)
    dec.close()
    return [(np.concatenate(pcm[s], axis=1), samp[s], stat[s]) for s in range(S)]


def decode_one(v, ds, packets, cuda):
    """one stream, one packet per call, with granulepos and eos -> decoded PCM [ch, n]"""
    pcm, _, status = stepwise(v, ds, [packets], cuda)[0]
    assert not any(status)
    return pcm


def linear(v, ds, pk, cuda):
    """the whole stream in one synthesis_runs call -> pcm [ch, total] (equal to the stepwise decode:
    tests/test_decode_runs_gpu.py)"""
    dec = v.Decoder(ds, 1, max(1, len(pk)))
    pcm, rs, _, _ = runs_call(dec, [0], [pk], cuda)
    out = pcm[0, :, :int(rs[0])].cpu().numpy()
    dec.close()
    return out


def ranges(dec, store, ids, starts, lengths):
    """one call into a buffer filled with FILL_RANGES -> (pcm numpy, got)"""
    L = max(1, max(lengths, default=0))
    out = torch.full((len(ids), dec.channels, L), FILL_RANGES, dtype=torch.float32, device="cuda")
    pcm, got = dec.synthesis_ranges(store, ids, starts, lengths, out=out)
    return pcm.cpu().numpy(), got


def check(lin, ids, starts, lengths, pcm, got, what=""):
    """`ranges`' output against the same slices of the streams' linear decodes"""
    for r, (i, s, L) in enumerate(zip(ids, starts, lengths)):
        n = max(0, min(lin[i].shape[1] - s, L))
        assert got[r] == n, f"{what} range {r}: got"
        assert np.array_equal(pcm[r, :, :n], lin[i][:, s:s + n]), f"{what} range {r} (stream {i}, start {s}, len {L})"
        assert np.all(pcm[r, :, n:] == FILL_RANGES), f"{what} range {r}: written past got"


class Collect:
    """per stream: the device outputs of calls, concatenated on the host at the end (one wait)"""

    def __init__(self, S):
        self.parts = [[] for _ in range(S)]

    def add(self, sid, pcm, nsamp, samples, status):
        self.parts[sid].append((pcm, nsamp, samples, status))

    def result(self, sid):
        pcm, samp, stat = [], [], []
        for p, n, sm, st in self.parts[sid]:
            n = int(n)
            pcm.append(p[:, :n].cpu().numpy())
            samp += sm.cpu().tolist()
            stat += st.cpu().tolist()
        return np.concatenate(pcm, axis=1), samp, stat

    def add_runs(self, ids, runs, out):
        pcm, rs, sm, st = out
        at = 0
        for r, sid in enumerate(ids):
            c = len(runs[r])
            self.add(sid, pcm[r], rs[r], sm[at:at + c], st[at:at + c])
            at += c

    def add_steps(self, ids, out):
        pcm, sm, st = out
        for r, sid in enumerate(ids):
            self.add(sid, pcm[r], sm[r], sm[r:r + 1], st[r:r + 1])


def assert_same(got, want, what=""):
    assert got[2] == want[2], f"{what}: status"
    assert got[1] == want[1], f"{what}: samples"
    assert got[0].dtype == np.float32 and np.array_equal(got[0], want[0]), f"{what}: pcm"


def against_model(dec, results, status, samples, what):
    """the intermediates of the last call against the model's results (tests/vorbis_model.py), row by row"""
    got = {n: dec.fetch(n).cpu().numpy() for n in ("info", "floor_used", "floor_index", "residue", "spectrum")}
    for k, r in enumerate(results):
        assert status[k] == r["status"], f"{what} row {k}: status"
        if r["status"]:
            assert samples[k] == 0 and not got["spectrum"][k].any(), f"{what} row {k}: a failed row gives nothing"
            continue
        assert list(got["info"][k]) == r["info"], f"{what} row {k}: info"
        assert np.array_equal(got["floor_used"][k], r["used"]), f"{what} row {k}: floor used"
        assert np.array_equal(got["floor_index"][k], r["floor_index"]), f"{what} row {k}: floor index"
        assert got["residue"][k].tobytes() == r["residue"].tobytes(), f"{what} row {k}: residue"
        assert got["spectrum"][k].tobytes() == r["spectrum"].tobytes(), f"{what} row {k}: spectrum"
    return got


# ---- real packets from the device encoder ----------------------------------------------------------------------------
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


def encode_chunked(v, setup, sig, cuda):
    """device front end, 1024 samples per write with the rounds drained in between, end of stream declared
    -> [(packet, granulepos, eos)] of the one stream"""
    enc = v.Encoder(setup, 1)
    fe = v.FrontEnd(enc)
    got = []

    def drain():
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                return
            packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
            for k, pi in enumerate(info):
                got.append((int(pi["packetno"]), bytes(packets[k, :nbytes[k]]), int(pi["granulepos"]), int(pi["eos"])))

    dsig = torch.from_numpy(np.ascontiguousarray(sig[None])).to(cuda)
    for c in range(0, sig.shape[1], 1024):
        fe.write(dsig[:, :, c:c + 1024].contiguous())
        drain()
    fe.finish()
    drain()
    fe.close()
    enc.close()
    got.sort()
    assert [g[0] for g in got] == list(range(3, 3 + len(got))) and got[-1][3] == 1
    return [g[1:] for g in got]


def encoded(v, setup, seconds, seed, cuda, burst=False):
    ch, rate = setup.channels, setup.rate
    n = int(seconds * rate) // 1024 * 1024
    sig = (burst_signal if burst else synth_signal)(ch, rate, n, seed=seed)
    return encode_chunked(v, setup, sig, cuda)


# ---- decoded PCM against a float64 and a float32 restatement --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cosines(N):
    k, t = np.arange(N // 2), np.arange(N)
    return np.cos(2 * np.pi / N * np.outer(t + 0.5 + N / 4, k + 0.5))


def imdct64(X):
    """float64 mdct_backward: C^T X with C[k, n] = cos(2 pi / N (n + 1/2 + N/4)(k + 1/2)) (the reference's forward is
    4/N C x; window, forward, backward, window and overlap-add return the input)"""
    return _cosines(2 * len(X)) @ X.astype(np.float64)


def overlap(tail, lW, p, W, n0, n1, w0, w1):
    """vorbis_synthesis_blockin's overlap-add (lib/block.c:897-1045) in the dtype of its arguments: what becomes final,
    and the new tail.  n0 / n1: half the two block sizes (a quarter at half rate), w0 / w1 the rising half windows of
    those lengths.  In float32 numpy rounds each product and the sum separately, as the scalar
    pcm[i]*w[n-i-1] + p[i]*w[i] does with contraction off"""
    n = n1 if W else n0
    if lW < 0:
        return np.zeros(0, p.dtype), p[n:2 * n].copy()
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
    assert out.dtype == p.dtype
    return out, p[n:2 * n].copy()


def final_pcm(ds, streams_pk, spec_steps, info_steps, samples_steps, hs, backward, w0, w1):
    """The walk both PCM checks make.  Per stream and step: backward(spectrum [ch, N/2]) -> [ch, N] points, N =
    blocksizes[W] >> hs, overlap-added (`overlap`) with the rising half windows w0 / w1 in their dtype, the tail
    carried.  Yields (stream, step, W, the W before or -1, want [ch, ns]): the yardstick's final samples, cut to the ns
    the device returned.  ns is the overlap's length, or less on a stream's last packet: the end-of-stream packet is
    trimmed to its granule position (lib/block.c:1084-1161) and the first ns stay"""
    bs = ds.blocksizes
    n0, n1 = bs[0] >> (1 + hs), bs[1] >> (1 + hs)
    assert (len(w0), len(w1)) == (n0, n1)
    for s in range(len(streams_pk)):
        tail, lW = None, -1
        for t in range(len(streams_pk[s])):
            W = int(info_steps[t][s][1])
            N = bs[W] >> hs
            p = backward(np.stack([spec_steps[t][s][c][:N // 2] for c in range(ds.channels)]))
            pairs = [overlap(tail[c] if tail is not None else None, lW, p[c], W, n0, n1, w0, w1) for c in range(ds.channels)]
            want, tail = np.stack([o for o, _ in pairs]), [tl for _, tl in pairs]
            assert lW < 0 or want.shape[1] == (bs[lW] // 4 + bs[W] // 4) >> hs
            ns = int(samples_steps[t][s])
            last = t == len(streams_pk[s]) - 1
            assert ns == want.shape[1] or (last and ns < want.shape[1]), (s, t, ns, want.shape[1])
            yield s, t, W, lW, want[:, :ns]
            lW = W


def check_pcm_bound(ds, streams_pk, pcm_steps, spec_steps, info_steps, samples_steps, win=None, peaks=None,
                    halfrate=False):
    """per stream: the device PCM of every step against float64 IMDCT + window + OLA of the fetched spectrum; at half
    rate the IMDCT of half the block size over the lower half of the bins (lib/block.c:208-209: the transform is made
    for blocksizes[W] >> hs).  Bound: 1e-5 of the step's float64 peak (of 1e-3 below that).
    win: the two windows' rising halves (default: the product's own table); peaks: a list that receives every step's
    float64 peak -> the worst error / peak"""
    import vorbis_aotuv_lancer_amd as v
    hs = 1 if halfrate else 0
    if win is None:
        win = [v.window_table(ds.blocksizes[0] >> hs), v.window_table(ds.blocksizes[1] >> hs)]
    worst = 0.0
    for s, t, _, _, want in final_pcm(ds, streams_pk, spec_steps, info_steps, samples_steps, hs,
                                      lambda spec: np.stack([imdct64(x) for x in spec]),
                                      win[0].astype(np.float64), win[1].astype(np.float64)):
        ns = want.shape[1]
        if ns:
            got = pcm_steps[t][s][:, :ns].astype(np.float64)
            if peaks is not None:
                peaks.append(float(np.abs(want).max()))
            peak = max(np.abs(want).max(), 1e-3)
            err = np.abs(got - want).max()
            worst = max(worst, err / peak)
            assert err <= 1e-5 * peak, f"stream {s} step {t}: max error {err} at peak {peak}"
    return worst


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
    w0, w1 = v.window_table(bs[0] >> hs), v.window_table(bs[1] >> hs)
    assert w0.dtype == np.float32 and w1.dtype == np.float32
    compared = 0
    for s, t, W, lW, want in final_pcm(ds, streams_pk, spec_steps, info_steps, samples_steps, hs,
                                       lambda spec: oracle.mdct_backward(np.asarray(spec, np.float32)), w0, w1):
        got = pcm_steps[t][s][:, :want.shape[1]]
        assert got.dtype == np.float32 and want.dtype == np.float32
        if not np.array_equal(got, want):
            c, i = (int(x[0]) for x in np.nonzero(got != want))
            raise AssertionError(
                f"stream {s} step {t} channel {c} sample {i} (block of {bs[W]}, after {'none' if lW < 0 else bs[lW]}"
                f"{', half rate' if hs else ''}): device {float(got[c, i]):.9g}, scalar inverse MDCT "
                f"{float(want[c, i]):.9g}, {ulps_apart(got[c, i], want[c, i])} ulps apart; "
                f"{int((got != want).sum())} of {got.size} differ")
        compared += 1 if want.shape[1] else 0
    return compared
