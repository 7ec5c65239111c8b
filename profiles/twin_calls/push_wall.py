#!/usr/bin/env python3
"""Wall time of the wrapper methods themselves, which tools/bench_feed.py and tools/bench_demux.py pass by with raw calls:
OggFeed.push per call (strict and resync; device, and the host twin) and demux_ogg_device per batch.  --root TREE: the
built tree to import the package from.  Prints one JSON line; times are medians over --reps passes after a warm-up."""
import argparse
import json
import statistics
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", required=True)
ap.add_argument("--slots", type=int, default=1024)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--reps", type=int, default=15)
a = ap.parse_args()
sys.path.insert(0, a.root)
import torch  # noqa: E402
import vorbis_aotuv_lancer_amd as v  # noqa: E402

rng = np.random.default_rng(11)
setup = v.Setup(2, 44100, 0.5)
files = []
for k in range(16):
    pk = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in np.clip(rng.normal(475, 150, 40), 1, 4000)]
    files.append(v.write_ogg(setup, pk, [(1024 * (i + 1), i == len(pk) - 1) for i in range(len(pk))], serialno=k + 1))
S, T = a.slots, a.calls
piece = [-(-len(f) // T) for f in files]
ids = np.arange(S, dtype=np.int32)


def calls(device):
    out = []
    for t in range(T):
        parts = [files[s % 16][t * piece[s % 16]:(t + 1) * piece[s % 16]] for s in range(S)]
        off = np.zeros(S + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        raw = np.frombuffer(b"".join(parts), np.uint8).copy()
        out.append((torch.from_numpy(raw).cuda() if device else raw, off, t == T - 1))
    return out


def per_push_us(host, resync):
    cs = calls(not host)
    feed = v.OggFeed(S, max(int(c[1][-1]) for c in cs), host=host, resync=resync)
    times = []
    for rep in range(a.reps + 1):
        feed.reset(ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for raw, off, end in cs:
            r = feed.push(ids, raw, end=end, offsets=off)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) / T * 1e6)
    assert not any(r.status)
    feed.close()
    return {"median": statistics.median(times), "series": times}


def demux_ms(**kw):
    times = []
    for rep in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = v.demux_ogg_device(files * 4, **kw)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    assert not any(b.status)
    return {"median": statistics.median(times), "series": times}


print(json.dumps({"metric": "wrapper_wall", "slots": S, "calls": T, "reps": a.reps,
                  "push_us": {"device_strict": per_push_us(False, False), "device_resync": per_push_us(False, True),
                              "host_strict": per_push_us(True, False), "host_resync": per_push_us(True, True)},
                  "demux_ogg_device_ms": {"plain": demux_ms(), "chained": demux_ms(chained=True),
                                          "multiplexed": demux_ms(multiplexed=True), "resync": demux_ms(resync=True)}}),
      flush=True)
