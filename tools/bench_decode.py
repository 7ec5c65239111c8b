#!/usr/bin/env python3
"""Decode measurement (outside bench.py): vbm_synthesis_batch at full size on one MI355X.

Packets come from the device encoder: K distinct signals are encoded by the front end (end of stream declared) and
dealt round robin to `--streams` decode streams, so every step mixes the block types of K different streams.  All
step inputs are built on the device first; then `--warmup` steps run, and `--steps` consecutive steps (one packet per
stream each, never synchronised with the host in between) are timed with device events.  Prints one JSON line:
ms per step, and the streams decoded at 1x realtime (decoded audio seconds / wall seconds).

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
    a = ap.parse_args()

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
    dec = v.Decoder(ds, S, S)
    half = ds.blocksizes[1] // 2
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
    audio_s = samples_sum / rate                          # per-channel samples summed over all streams
    res = {
        "metric": "decode_step_ms", "streams": S, "signals": K, "channels": ch, "rate": rate, "quality": a.quality,
        "steps": a.steps, "ms_per_step": ms / a.steps, "realtime_streams": audio_s / (ms / 1e3),
        "packet_bytes_per_step": sum(nbytes_step[a.warmup:]) / a.steps, "status_errors": int(bad),
        "blocksizes": list(ds.blocksizes),
    }
    print(json.dumps(res))
    dec.close()
    ds.close()


if __name__ == "__main__":
    main()
