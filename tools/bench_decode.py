#!/usr/bin/env python3
"""Decode measurement (outside bench.py): vbm_synthesis_batch at full size on one MI355X.

Packets come from the device encoder: K distinct signals are encoded by the front end (end of stream declared) and
dealt round robin to `--streams` decode streams, so every step mixes the block types of K different streams.  All
step inputs are built on the device first; then `--warmup` steps run, and `--steps` consecutive steps (one packet per
stream each, never synchronised with the host in between) are timed with device events.  Prints one JSON line:
ms per step, and the streams decoded at 1x realtime (decoded audio seconds / wall seconds).

With --packets-per-call P > 1 the same workload goes through vbm_synthesis_runs instead: each call takes P
consecutive packets of every stream (P * (warmup + steps) packets per stream are needed: raise --seconds), and the
result reports ms per call and per packet-step (ms per call / P).  P = 1 (the default) is the one-packet path above.

With --ranges N the store of seekable range decoding is measured instead (vbm_synthesis_ranges): the `--streams`
streams (the encoded signals dealt round robin) go into one range store, and every call decodes N seeded random
(stream, start) windows of --range-seconds each.  The result reports ms per call, ranges/s, audio seconds decoded per
wall second, rows per call and the pre-roll share of those rows (from the host index).

With --halfrate the decoder is a half-rate one (Decoder(..., halfrate=True)) in any of the three modes:
the same packets, half as many output samples at rate / 2; range windows are --range-seconds of output.

Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--signals", type=int, default=64, help="distinct signals (encoded streams) dealt round robin")
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--quality", type=float, default=0.5)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--packets-per-call", type=int, default=1,
                    help="P > 1: P consecutive packets per stream per call through synthesis_runs")
    ap.add_argument("--ranges", type=int, default=0, help="N > 0: N random windows per call through synthesis_ranges")
    ap.add_argument("--range-seconds", type=float, default=1.0, help="length of each window (--ranges)")
    ap.add_argument("--max-batch", type=int, default=65536, help="rows per sub-call of a range call (--ranges)")
    ap.add_argument("--halfrate", action="store_true", help="decode at half the sample rate (with any of the modes)")
    a = ap.parse_args()
    P = a.packets_per_call
    if P < 1:
        raise SystemExit("--packets-per-call must be at least 1")

    import vorbis_aotuv_lancer_amd as v
    from tests.signals import synth_signal

    dev = torch.device("cuda:0")
    S, K, ch, rate = a.streams, a.signals, a.channels, a.rate
    setup = v.Setup(ch, rate, a.quality)
    nsamp = int(a.seconds * rate) // 1024 * 1024
    sigs = np.stack([synth_signal(ch, rate, nsamp, seed=300 + k, level=1.0 if k % 4 else 0.05) for k in range(K)])
    enc = v.Encoder(setup, K)
    fe = v.FrontEnd(enc)
    lead = [[] for _ in range(K)]

    def drain():
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                return
            packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
            for r, pi in enumerate(info):
                lead[int(pi["stream"])].append((int(pi["packetno"]), bytes(packets[r, :nbytes[r]]),
                                                int(pi["granulepos"]), int(pi["eos"])))

    dsig = torch.from_numpy(sigs).to(dev)
    for c in range(0, nsamp, 1024):
        fe.write(dsig[:, :, c:c + 1024].contiguous())
        drain()
    fe.finish()
    drain()
    fe.close()
    enc.close()
    for x in lead:
        x.sort()
    nsteps = a.warmup + a.steps
    if a.ranges > 0:
        return ranges(a, v, dev, setup, lead)
    if P > 1:
        return runs(a, v, dev, setup, lead)
    if min(len(x) for x in lead) < nsteps:
        raise SystemExit(f"need {nsteps} packets per stream, have {min(len(x) for x in lead)}: raise --seconds")
    stride = max(len(p[1]) for x in lead for p in x[:nsteps])
    lp = np.zeros((K, nsteps, stride), np.uint8)
    lnb = np.zeros((K, nsteps), np.int32)
    lgp = np.zeros((K, nsteps), np.int64)
    for k in range(K):
        for t in range(nsteps):
            _, p, gp, _ = lead[k][t]
            lp[k, t, :len(p)] = np.frombuffer(p, np.uint8)
            lnb[k, t], lgp[k, t] = len(p), gp
    lp, lnb, lgp = (torch.from_numpy(x).to(dev) for x in (lp, lnb, lgp))
    ids = np.arange(S, dtype=np.int32)
    li = torch.from_numpy(ids % K).to(dev)
    inputs = [(lp[li, t].contiguous(), lnb[li, t].contiguous(), lgp[li, t].contiguous()) for t in range(nsteps)]
    nbytes_step = [float(lnb[li, t].sum()) for t in range(nsteps)]

    ds = v.DecodeSetup(v.header_packets(setup))
    dec = v.Decoder(ds, S, S, halfrate=a.halfrate)
    half = dec.row
    pcm = [torch.empty((S, ch, half), dtype=torch.float32, device=dev) for _ in range(2)]
    outs = [(pcm[t % 2], torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S, dtype=torch.int32, device=dev))
            for t in range(nsteps)]
    for t in range(a.warmup):
        pk, nb, gp = inputs[t]
        dec.synthesis_batch(ids, pk, nb, granulepos=gp, out=outs[t])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(a.warmup, nsteps):                     # nothing but the decode calls between the events
        pk, nb, gp = inputs[t]
        dec.synthesis_batch(ids, pk, nb, granulepos=gp, out=outs[t])
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    samples_sum = sum(int(outs[t][1].sum()) for t in range(a.warmup, nsteps))
    bad = sum(int((outs[t][2] != 0).sum()) for t in range(nsteps))
    audio_s = samples_sum / dec.rate                      # per-channel samples summed over all streams
    res = {
        "metric": "decode_step_ms", "halfrate": bool(a.halfrate), "streams": S, "signals": K, "channels": ch, "rate": rate, "quality": a.quality,
        "steps": a.steps, "ms_per_step": ms / a.steps, "realtime_streams": audio_s / (ms / 1e3),
        "packet_bytes_per_step": sum(nbytes_step[a.warmup:]) / a.steps, "status_errors": int(bad),
        "blocksizes": list(ds.blocksizes),
    }
    print(json.dumps(res))
    dec.close()
    ds.close()


def runs(a, v, dev, setup, lead):
    """the same workload, P packets per stream per call (vbm_synthesis_runs)"""
    S, K, ch, rate, P = a.streams, a.signals, a.channels, a.rate, a.packets_per_call
    ncalls = a.warmup + a.steps
    if S % K:
        raise SystemExit("--streams must be a multiple of --signals with --packets-per-call > 1")
    if min(len(x) for x in lead) < P * ncalls:
        raise SystemExit(f"need {P * ncalls} packets per stream, have {min(len(x) for x in lead)}: raise --seconds")
    inputs, nbytes_call = [], []
    for c in range(ncalls):                               # stream s reads lead s % K: the K leads tiled S // K times
        data, offs, gps, base = [], [np.zeros(1, np.int64)], [], 0
        for k in range(K):
            seg = lead[k][c * P:(c + 1) * P]
            b = b"".join(p[1] for p in seg)
            data.append(np.frombuffer(b, np.uint8))
            offs.append(np.cumsum([len(p[1]) for p in seg]).astype(np.int64) + base)
            gps.append(np.array([p[2] for p in seg], np.int64))
            base += len(b)
        one = np.concatenate(data)
        o1 = np.concatenate(offs)
        reps = S // K
        offsets = np.concatenate([np.zeros(1, np.int64)] + [o1[1:] + r * base for r in range(reps)])
        inputs.append((torch.from_numpy(np.tile(one, reps)).to(dev), torch.from_numpy(offsets).to(dev),
                       torch.from_numpy(np.tile(np.concatenate(gps), reps)).to(dev)))
        nbytes_call.append(float(base * reps))
    ds = v.DecodeSetup(v.header_packets(setup))
    dec = v.Decoder(ds, S, S * P, halfrate=a.halfrate)
    half = dec.row
    ids = np.arange(S, dtype=np.int32)
    counts = np.full(S, P, np.int32)
    pcm = [torch.empty((S, ch, P * half), dtype=torch.float32, device=dev) for _ in range(2)]
    outs = [(pcm[c % 2], torch.empty(S, dtype=torch.int32, device=dev), torch.empty(S * P, dtype=torch.int32, device=dev),
             torch.empty(S * P, dtype=torch.int32, device=dev)) for c in range(ncalls)]
    for c in range(a.warmup):
        data, offs, gp = inputs[c]
        dec.synthesis_runs(ids, counts, data, offs, granulepos=gp, out=outs[c])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for c in range(a.warmup, ncalls):                     # nothing but the decode calls between the events
        data, offs, gp = inputs[c]
        dec.synthesis_runs(ids, counts, data, offs, granulepos=gp, out=outs[c])
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    samples_sum = sum(int(outs[c][1].sum()) for c in range(a.warmup, ncalls))
    bad = sum(int((outs[c][3] != 0).sum()) for c in range(ncalls))
    audio_s = samples_sum / dec.rate
    res = {
        "metric": "decode_runs_ms", "halfrate": bool(a.halfrate), "streams": S, "signals": K, "channels": ch, "rate": rate, "quality": a.quality,
        "packets_per_call": P, "calls": a.steps, "ms_per_call": ms / a.steps, "ms_per_packet_step": ms / a.steps / P,
        "realtime_streams": audio_s / (ms / 1e3), "packet_bytes_per_call": sum(nbytes_call[a.warmup:]) / a.steps,
        "status_errors": int(bad), "blocksizes": list(ds.blocksizes),
    }
    print(json.dumps(res))
    dec.close()
    ds.close()


def ranges(a, v, dev, setup, lead):
    """random sample windows of a range store of --streams streams (vbm_synthesis_ranges)"""
    S, K, ch, rate, N = a.streams, a.signals, a.channels, a.rate, a.ranges
    L = int(a.range_seconds * rate) // (2 if a.halfrate else 1)       # samples at the output rate
    streams = []
    for k in range(K):
        b = b"".join(p[1] for p in lead[k])
        streams.append((np.frombuffer(b, np.uint8), np.cumsum([0] + [len(p[1]) for p in lead[k]]).astype(np.int64),
                        np.array([p[2] for p in lead[k]], np.int64), np.array([p[3] for p in lead[k]], np.uint8)))
    ds = v.DecodeSetup(v.header_packets(setup))
    index = [v.decode_index(ds, *s, halfrate=a.halfrate) for s in streams]
    dec = v.Decoder(ds, 1, a.max_batch, halfrate=a.halfrate)
    store = v.RangeStore(dec, [streams[s % K] for s in range(S)])
    rng = np.random.default_rng(1234)
    ncalls = a.warmup + a.steps
    calls, rows, preroll = [], 0, 0
    for c in range(ncalls):
        ids = rng.integers(0, S, N).astype(np.int32)
        starts = (rng.random(N) * np.maximum(store.totals[ids] - L, 1)).astype(np.int64)
        calls.append((ids, starts))
        if c >= a.warmup:                                  # rows of the plan, from the host index
            for i, s in zip(ids, starts):
                status, samples, out_start, total = index[i % K]
                n = min(L, total - s)
                if n <= 0:
                    continue
                out_end = out_start + samples
                k = int(np.searchsorted(out_end, s, side="right"))
                m = int(np.searchsorted(out_end, s + n - 1, side="right"))
                p = k - 1
                while status[p] != 0:
                    p -= 1
                rows += m - p + 1
                preroll += 1
    pcm = [torch.empty((N, ch, L), dtype=torch.float32, device=dev) for _ in range(2)]
    lengths = np.full(N, L, np.int32)
    for c in range(a.warmup):
        dec.synthesis_ranges(store, calls[c][0], calls[c][1], lengths, out=pcm[c % 2])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    got_sum = 0
    for c in range(a.warmup, ncalls):                     # the range calls only (the host plans each call)
        _, got = dec.synthesis_ranges(store, calls[c][0], calls[c][1], lengths, out=pcm[c % 2])
        got_sum += int(got.sum())
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    res = {
        "metric": "decode_ranges_ms", "halfrate": bool(a.halfrate), "streams": S, "signals": K, "channels": ch, "rate": rate, "quality": a.quality,
        "ranges_per_call": N, "range_seconds": a.range_seconds, "max_batch": a.max_batch, "calls": a.steps,
        "ms_per_call": ms / a.steps, "ranges_per_s": N * a.steps / (ms / 1e3),
        "audio_s_per_wall_s": got_sum / dec.rate / (ms / 1e3), "rows_per_call": rows / a.steps,
        "preroll_share": preroll / max(rows, 1), "blocksizes": list(ds.blocksizes),
    }
    print(json.dumps(res))
    store.close()
    dec.close()
    ds.close()


if __name__ == "__main__":
    main()
