#!/usr/bin/env python3
"""Live range store measurement (outside bench.py), on one MI355X.  Prints one JSON line per fill level.

`--slots` stereo q5 slots (default 4096) are fed the packets of one encoded signal, round and round, every slot from
its own place in it, `--run` packets per slot per append (8 packets are about 0.19 s of audio).  For each `--fills`
value F the store is LiveRangeStore(dec, slots, max_packets=F, max_bytes=F * the largest packet), filled with a seeded
number of packets per slot so that the slots do not trim in step, and then appended to until every slot has trimmed:
    append_ms     wall time of one LiveRangeStore.append over all slots (the call ends in its one wait for the device):
                  median, quartiles and extremes over --reps appends in the steady state, after --warmup more;
                  trims_per_append says how many slots trimmed per timed call on average
    rebuild_ms    the only alternative without the store: RangeStore.from_device over a CSR of as many packets per slot
                  as the store retains on average (the same packet sequence, every slot from its start), wall time,
                  median of --rebuild-reps after one warm-up; what a caller would pay per request
Two fill levels show whether an append grows with the history kept.  Nothing here is a pass mark."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median": round(statistics.median(ms), 4), "q1": round(q[0], 4), "q3": round(q[2], 4),
            "min": round(min(ms), 4), "max": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--run", type=int, default=8)
    ap.add_argument("--fills", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rebuild-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    a = ap.parse_args()
    import torch
    import vorbis_aotuv_lancer_amd as v
    from tests.signals import synth_signal
    if not torch.cuda.is_available():
        sys.exit("bench_live_store needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    blob = v.encode_ogg([synth_signal(2, 44100, int(a.seconds * 44100), seed=a.seed)], 44100, quality=0.5)[0]
    headers, data, offsets, _, _ = v.demux_ogg(blob)
    data, offsets = np.asarray(data, np.uint8), np.asarray(offsets, np.int64)
    N, sizes = len(offsets) - 1, np.diff(offsets)
    ds = v.DecodeSetup(headers)
    dec = v.Decoder(ds, a.slots, 1024)
    rng = np.random.default_rng(a.seed)
    phase = rng.integers(0, N, a.slots)
    cycle = np.concatenate([data, data])                  # any run of up to N packets is contiguous in it
    off2 = np.concatenate([offsets, offsets[1:] + offsets[-1]])

    def call(counts):
        """the next counts[s] packets of every slot as one CSR on the device -> (counts, payload, offsets)"""
        parts, lens = [], []
        for s, c in enumerate(counts):
            p = int(phase[s])
            parts.append(cycle[off2[p]:off2[p + c]])
            lens.append(np.diff(off2[p:p + c + 1]))
            phase[s] = (p + c) % N
        offs = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
        return counts, torch.from_numpy(np.concatenate(parts)).to(dev), torch.from_numpy(offs).to(dev)

    ids = np.arange(a.slots, dtype=np.int32)
    for F in a.fills:
        store = v.LiveRangeStore(dec, a.slots, F, F * int(sizes.max()))
        left = rng.integers(0, F // 2, a.slots)                            # the seeded fill: slots do not trim in step
        while left.any():
            counts = np.minimum(left, min(N, F))
            left -= counts
            store.append(ids, *call(counts))
        calls = [call(np.full(a.slots, a.run)) for _ in range(a.warmup + a.reps)]   # built outside the timing
        need = F // a.run + 1                                              # appends until every slot has trimmed once
        for k in range(need):
            store.append(ids, *call(np.full(a.slots, a.run)))
        torch.cuda.synchronize()
        ms, before = [], None
        for k, c in enumerate(calls):
            if k == a.warmup:
                before = sum(store.stats.values())
            t0 = time.perf_counter()
            store.append(ids, *c)
            ms.append((time.perf_counter() - t0) * 1e3)
        trims = (sum(store.stats.values()) - before) / a.reps
        fill = int(store.packets.mean())
        # the alternative: a store built over the same number of packets per slot, per request
        one = np.diff(off2[:fill + 1]) if fill <= N else np.resize(sizes, fill)
        payload = torch.from_numpy(np.resize(np.concatenate([data] * (fill // N + 1)), int(one.sum()))).to(dev).repeat(a.slots)
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(np.tile(one, a.slots))]).astype(np.int64)).to(dev)
        first = np.arange(a.slots + 1, dtype=np.int64) * fill
        rb = []
        for k in range(a.rebuild_reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rs = v.RangeStore.from_device(dec, payload, offs, stream_packets=first)
            rb.append((time.perf_counter() - t0) * 1e3)
            rs.close()
        line = json.dumps({"bench": "live_store", "slots": a.slots, "run_packets": a.run, "max_packets": F,
                           "retained_packets_mean": fill, "retained_MiB": round(float(store.bytes.sum()) / 2 ** 20, 1),
                           "append_ms": spread(ms[a.warmup:]), "trims_per_append": round(trims, 1),
                           "rebuild_ms": spread(rb[1:]), "device": torch.cuda.get_device_name(0)})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del payload, offs
        store.close()
    dec.close()
    ds.close()


if __name__ == "__main__":
    main()
