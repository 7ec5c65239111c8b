#!/usr/bin/env python3
"""Decode measurement over several header classes (outside bench.py): K per-class Decoder calls per step against one
MixedDecoder call, on one MI355X.

`--streams` decode streams are spread evenly over `--classes` K header classes: stereo mode packs of different
qualities and rates (CLASSES below, in that order), so every class has stereo-q5-sized packets and the block sizes
256 / 2048.  Per class `--signals` distinct signals are encoded by the device encoder and dealt round robin to the
class's streams.  A step is `--packets-per-call` P consecutive packets of every stream: through synthesis_batch at
P = 1 and synthesis_runs at P > 1, the settings of tools/bench_decode.py.  All inputs are built on the device first.
Then, per step, with device events around each and no host wait inside:
  (a) per_class  K calls, one per class, each on that class's own Decoder: what a caller does without a MixedDecoder
  (b) mixed      one call of one MixedDecoder whose caps are those of the classes (2 channels, blocks of 2048)
(a) and (b) alternate step by step and decode the same packets into their own outputs; after `--warmup` steps the
medians over `--steps` steps are reported, with the device memory per row of both kinds of decoder.  On a tree without
MixedDecoder only (a) runs.  With --caps-max the mixed decoder has the largest caps instead (8 channels, blocks of
4096): the price of padding.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = [(44100, 0.5), (48000, 0.5), (44100, 0.8), (48000, 0.1), (44100, 0.1), (48000, 0.8), (44100, 0.4), (48000, 0.6),
           (44100, 0.6), (48000, 0.4), (44100, 0.7), (48000, 0.7), (44100, 0.9), (48000, 0.9), (44100, 0.0), (48000, 0.0)]


def encode_class(v, dev, rate, quality, nsig, seconds):
    """-> (header packets, per signal [(packet, granulepos)]) of nsig stereo signals through the device encoder"""
    from tests.signals import synth_signal
    setup = v.Setup(2, rate, quality)
    nsamp = int(seconds * rate) // 1024 * 1024
    sigs = np.stack([synth_signal(2, rate, nsamp, seed=300 + k, level=1.0 if k % 4 else 0.05) for k in range(nsig)])
    enc = v.Encoder(setup, nsig)
    fe = v.FrontEnd(enc)
    lead = [[] for _ in range(nsig)]

    def drain():
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                return
            packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
            for r, pi in enumerate(info):
                lead[int(pi["stream"])].append((int(pi["packetno"]), bytes(packets[r, :nbytes[r]]), int(pi["granulepos"])))

    dsig = torch.from_numpy(sigs).to(dev)
    for c in range(0, nsamp, 1024):
        fe.write(dsig[:, :, c:c + 1024].contiguous())
        drain()
    fe.finish()
    drain()
    fe.close()
    enc.close()
    headers = v.header_packets(setup)
    return headers, [[(p, gp) for _, p, gp in sorted(x)] for x in lead]


def step_inputs(dev, leads, streams, at, P):
    """the rows of one step for `streams` [(class, signal)]: packets at .. at + P of each
    -> (data uint8, offsets int64 [n P + 1], granulepos int64 [n P]) on the device"""
    segs = [leads[c][k][at:at + P] for c, k in streams]
    lens = np.array([len(p) for seg in segs for p, _ in seg], np.int64)
    data = np.frombuffer(b"".join(p for seg in segs for p, _ in seg), np.uint8).copy()
    offs = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])
    gps = np.array([gp for seg in segs for _, gp in seg], np.int64)
    return tuple(torch.from_numpy(x).to(dev) for x in (data, offs, gps))


def padded(data, offs):
    """a one-packet-per-row CSR -> (packets uint8 [n, stride], nbytes int32 [n]) for synthesis_batch"""
    nb = (offs[1:] - offs[:-1]).to(torch.int32)
    stride = int(nb.max())
    col = torch.arange(stride, device=data.device)
    idx = (offs[:-1, None] + col[None, :]).clamp(max=data.numel() - 1)
    return (data[idx] * (col[None, :] < nb[:, None])).to(torch.uint8).contiguous(), nb.contiguous()


class Job:
    """one decoder, its streams, its per-step inputs and its output buffers"""

    def __init__(self, dec, ids, channels, row, P, inputs, dev):
        self.dec, self.ids, self.P, self.inputs = dec, np.asarray(ids, np.int32), P, inputs
        n = len(ids)
        self.counts = np.full(n, P, np.int32)
        self.pcm = torch.empty((n, channels, P * row), dtype=torch.float32, device=dev)
        self.ints = [torch.empty(k, dtype=torch.int32, device=dev) for k in (n, n * P, n * P)]
        if P == 1:
            self.inputs = [padded(d, o) + (g,) for d, o, g in inputs]

    def call(self, t):
        if self.P == 1:
            pk, nb, gp = self.inputs[t]
            self.dec.synthesis_batch(self.ids, pk, nb, granulepos=gp, out=(self.pcm, self.ints[0], self.ints[1]))
        else:
            data, offs, gp = self.inputs[t]
            self.dec.synthesis_runs(self.ids, self.counts, data, offs, granulepos=gp, out=(self.pcm, *self.ints))

    def errors(self):
        return int((self.ints[2 if self.P > 1 else 1] != 0).sum())


def timed(jobs, t):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for j in jobs:
        j.call(t)
    e1.record()
    return e0, e1


def row_bytes(channels, blocksize, halfrate):
    """device memory of one row of a call (residue, spectrum, IMDCT, floor posts, partition classes, flags, PCM of one
    packet) and of one stream (the tail), of a decoder with such rows"""
    half, hs = blocksize // 2, int(halfrate)
    row = channels * (2 * half * 4 + (blocksize >> hs) * 4 + 65 * 4 + 4) + channels * half + 4 * 10
    return {"per_row": row, "per_stream_tail": channels * (half >> hs) * 4, "pcm_per_packet": channels * (half >> hs) * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--classes", type=int, default=4, help=f"header classes, 1..{len(CLASSES)}")
    ap.add_argument("--signals", type=int, default=8, help="distinct signals per class, dealt round robin")
    ap.add_argument("--seconds", type=float, default=0.0, help="length of each signal (0: what the steps need)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--packets-per-call", type=int, default=1)
    ap.add_argument("--halfrate", action="store_true")
    ap.add_argument("--caps-max", action="store_true", help="mixed decoder with max_channels=8, max_blocksize=4096")
    a = ap.parse_args()
    import vorbis_aotuv_lancer_amd as v
    dev = torch.device("cuda:0")
    S, K, P, nsteps = a.streams, a.classes, a.packets_per_call, a.warmup + a.steps
    if not 1 <= K <= len(CLASSES) or S % K or (S // K) % a.signals:
        raise SystemExit("--streams must be a multiple of --classes x --signals, and --classes within the list")
    need = P * nsteps
    seconds = a.seconds or (need + 8) * 1024 / 44100           # a packet per 1024 samples at the least
    encoded = [encode_class(v, dev, rate, q, a.signals, seconds) for rate, q in CLASSES[:K]]
    leads = [x[1] for x in encoded]
    short = min(len(x) for lead in leads for x in lead)
    if short < need:
        raise SystemExit(f"need {need} packets per stream, have {short}: raise --seconds")
    per = S // K
    streams = [(c, s % a.signals) for c in range(K) for s in range(per)]        # stream c * per + s is of class c
    setups = [v.DecodeSetup(h) for h, _ in encoded]
    jobs_a = []
    for c in range(K):
        mine = streams[c * per:(c + 1) * per]
        inputs = [step_inputs(dev, leads, mine, t * P, P) for t in range(nsteps)]
        dec = v.Decoder(setups[c], per, per * P, halfrate=a.halfrate)
        jobs_a.append(Job(dec, range(per), 2, dec.row, P, inputs, dev))
    jobs_b = []
    if hasattr(v, "MixedDecoder"):
        caps = dict(max_channels=8, max_blocksize=4096) if a.caps_max else dict(max_channels=2, max_blocksize=2048)
        md = v.MixedDecoder(S, S * P, max_classes=K, halfrate=a.halfrate, **caps)
        for c in range(K):
            md.bind(list(range(c * per, (c + 1) * per)), [md.add_class(setups[c])] * per)
        inputs = [step_inputs(dev, leads, streams, t * P, P) for t in range(nsteps)]
        jobs_b.append(Job(md, range(S), md.channels, md.row, P, inputs, dev))
    torch.cuda.synchronize()
    ev_a, ev_b = [], []
    for t in range(nsteps):
        ev_a.append(timed(jobs_a, t))
        if jobs_b:
            ev_b.append(timed(jobs_b, t))
    torch.cuda.synchronize()
    ms = lambda ev: [e0.elapsed_time(e1) for e0, e1 in ev[a.warmup:]]         # noqa: E731
    res = {"metric": "decode_mixed_step_ms", "streams": S, "classes": K, "signals": a.signals, "packets_per_call": P,
           "halfrate": bool(a.halfrate), "steps": a.steps, "caps_max": bool(a.caps_max),
           "class_list": CLASSES[:K], "per_class_ms": ms(ev_a), "per_class_median_ms": float(np.median(ms(ev_a))),
           "status_errors": sum(j.errors() for j in jobs_a + jobs_b),
           "row_bytes_decoder": row_bytes(2, 2048, a.halfrate)}
    if jobs_b:
        res.update(mixed_ms=ms(ev_b), mixed_median_ms=float(np.median(ms(ev_b))),
                   row_bytes_mixed=row_bytes(md.channels, md.max_blocksize, a.halfrate),
                   row_bytes_mixed_at_largest_caps=row_bytes(8, 4096, a.halfrate))
        ja, jb = jobs_a[0], jobs_b[0]                          # the last step's PCM of class 0, sample for sample
        n = ja.ints[0].long()
        live = torch.arange(ja.pcm.shape[2], device=dev)[None, None, :] < n[:, None, None]
        zero = torch.zeros((), device=dev)
        same = torch.equal(n, jb.ints[0][:per].long()) and torch.equal(
            torch.where(live, ja.pcm, zero), torch.where(live, jb.pcm[:per, :2, :ja.pcm.shape[2]], zero))
        res["last_step_class0_pcm_equal"] = bool(same)
    print(json.dumps(res))
    for j in jobs_a + jobs_b:
        j.dec.close()
    for ds in setups:
        ds.close()


if __name__ == "__main__":
    main()
