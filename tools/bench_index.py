#!/usr/bin/env python3
"""Time to open an OggIndex (outside bench.py), on one MI355X: the host path (demux_ogg file by file, the index walked
on the host, packets uploaded) against device_demux=True (one upload of the files, the device demux, the store and its
index built on the device).  The two corpora of tools/bench_demux.py:
    files   `--files` stereo q5 files of seeded lengths between --min-seconds and --max-seconds, made by encode_ogg
    single  one file of about --single-mb MB: packets of random bytes with the sizes of stereo q5 packets, paged by
            write_ogg (the index reads only each packet's header bits, so random bytes give valid and failed packets)
Wall time around a device synchronise, upload included; the two paths alternate, --runs each after one warm-up round,
and their total_samples must be equal.  Prints one JSON line per corpus.  --paths device (or host) opens through one
path only, for a kernel trace of it."""
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


def open_report(v, name, files, runs, paths):
    times = {p: [] for p in paths}
    totals = {}
    packets = 0
    for rep in range(runs + 1):                            # the first round warms up
        for p in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            idx = v.OggIndex(files, device_demux=(p == "device"))
            torch.cuda.synchronize()
            if rep:
                times[p].append(time.perf_counter() - t0)
            totals[p] = idx.total_samples.copy()
            packets = int(idx.store.packets[-1])
            idx.close()
    if len(paths) == 2:
        assert np.array_equal(totals["host"], totals["device"]), f"{name}: total_samples differ between the two paths"
    nbytes = sum(len(f) for f in files)
    out = {"metric": "ogg_index_open", "corpus": name, "files": len(files), "ogg_bytes": nbytes, "packets": packets,
           "total_samples": int(totals[paths[0]].sum()), "runs": runs}
    for p in paths:
        med = statistics.median(times[p])
        out[p] = {"wall_s": med, "runs_s": times[p], "GB_per_s": nbytes / med / 1e9}
    if len(paths) == 2:
        out["speedup"] = out["host"]["wall_s"] / out["device"]["wall_s"]
        out["same_total_samples"] = True
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=6.0)
    ap.add_argument("--signals", type=int, default=16, help="distinct signals the files are cut from")
    ap.add_argument("--single-mb", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--paths", choices=["both", "host", "device"], default="both")
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_index.py needs a GPU: there is nothing to measure without one")
    if a.runs < 1:
        sys.exit("--runs must be at least 1")

    import vorbis_aotuv_lancer_amd as v
    from tests.signals import burst_signal

    paths = ["host", "device"] if a.paths == "both" else [a.paths]
    rate, rng = 44100, np.random.default_rng(a.seed)
    lengths = rng.integers(int(a.min_seconds * rate), int(a.max_seconds * rate) + 1, a.files)
    base = [burst_signal(2, rate, int(lengths.max()), seed=700 + k, period=20000, level=1.0 if k % 4 else 0.05)
            for k in range(a.signals)]
    files = v.encode_ogg([base[i % a.signals][:, :int(n)] for i, n in enumerate(lengths)], rate, quality=0.5)
    open_report(v, "files", files, a.runs, paths)

    setup = v.Setup(2, rate, 0.5)
    sizes = np.clip(rng.normal(475, 150, int(a.single_mb * 1e6 / 475)), 1, 4000).astype(int)
    packets = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in sizes]
    single = v.write_ogg(setup, packets, [(1024 * (k + 1), k == len(packets) - 1) for k in range(len(packets))])
    open_report(v, "single", [single], a.runs, paths)


if __name__ == "__main__":
    main()
