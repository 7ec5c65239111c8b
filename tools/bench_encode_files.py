#!/usr/bin/env python3
"""Whole-file encode measurement (outside bench.py): `--files` stereo q5 files of seeded lengths between --min-seconds
and --max-seconds through encode_ogg on one MI355X, over `--max-streams` slots.

The same workload runs twice per repetition, alternating:
    ragged    encode_ogg as it is: one FrontEnd.write_ragged per step, straight from the store of whole files
    grouped   the same driver with the step's write done as a caller had to before write_ragged existed: the listed
              slots grouped by write size, one stack of their slices and one FrontEnd.write_streams per distinct size
Everything else (schedule, rounds, paging, downloads) is shared, and the outputs of the two are compared byte for byte.
Wall time per run covers the whole call: upload of the store, every step, and the pages coming back.  Prints one JSON
line: files/s and audio seconds per wall second of both ways (median over --reps, after one warm-up run each), and
the write calls each way issued."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--max-streams", type=int, default=128)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=6.0)
    ap.add_argument("--signals", type=int, default=16, help="distinct signals the files are cut from")
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--quality", type=float, default=0.5)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()

    from vorbis_aotuv_lancer_amd import files as vf
    from tests.signals import burst_signal

    ch, rate = a.channels, a.rate
    rng = np.random.default_rng(a.seed)
    lengths = rng.integers(int(a.min_seconds * rate), int(a.max_seconds * rate) + 1, a.files)
    longest = int(lengths.max())
    base = [burst_signal(ch, rate, longest, seed=700 + k, period=20000, level=1.0 if k % 4 else 0.05)
            for k in range(a.signals)]
    pcms = [base[i % a.signals][:, :int(n)] for i, n in enumerate(lengths)]
    calls = {"ragged": 0, "grouped": 0}

    def ragged(fe, store, slots, file_ids, at, vals):
        calls["ragged"] += 1
        vf._write_ragged(fe, store, slots, file_ids, at, vals)

    def grouped(fe, store, slots, file_ids, at, vals):
        for n in sorted(set(vals)):
            ks = [k for k in range(len(slots)) if vals[k] == n]
            rows = [store.data[store.base[file_ids[k]]:store.base[file_ids[k]] + ch * store.stride[file_ids[k]]]
                    .view(ch, -1)[:, at[k]:at[k] + n] for k in ks]
            calls["grouped"] += 1
            fe.write_streams([slots[k] for k in ks], torch.stack(rows).contiguous())

    def run(write):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = vf._run_files(pcms, rate, a.quality, None, a.chunk, a.max_streams, None, (), write)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    ways = {"ragged": ragged, "grouped": grouped}
    outs = {name: run(w)[1] for name, w in ways.items()}               # warm-up, and the outputs to compare
    same = outs["ragged"] == outs["grouped"]
    for k in calls:
        calls[k] = 0
    times = {name: [] for name in ways}
    for _ in range(a.reps):
        for name, w in ways.items():
            times[name].append(run(w)[0])
    audio_s = float(lengths.sum()) / rate
    res = {"metric": "encode_files", "files": a.files, "max_streams": a.max_streams, "channels": ch, "rate": rate,
           "quality": a.quality, "chunk": a.chunk, "seconds": [a.min_seconds, a.max_seconds], "audio_seconds": audio_s,
           "ogg_bytes": sum(len(x) for x in outs["ragged"]), "same_bytes": bool(same), "reps": a.reps}
    for name in ways:
        t = statistics.median(times[name])
        res[name] = {"wall_s": t, "runs_s": times[name], "files_per_s": a.files / t, "audio_s_per_s": audio_s / t,
                     "write_calls_per_run": calls[name] // a.reps}
    res["speedup"] = res["grouped"]["wall_s"] / res["ragged"]["wall_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
