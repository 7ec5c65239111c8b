#!/usr/bin/env python3
"""Time to open an OggIndex (outside bench.py), on one MI355X: the host path (demux_ogg file by file, the index walked
on the host, packets uploaded) against device_demux=True (one upload of the files, the device demux, the store and its
index built on the device).  The two corpora of tools/bench_demux.py:
    files   `--files` stereo q5 files of seeded lengths between --min-seconds and --max-seconds, made by encode_ogg
    single  one file of about --single-mb MB: packets of random bytes with the sizes of stereo q5 packets, paged by
            write_ogg (the index reads only each packet's header bits, so random bytes give valid and failed packets)
Wall time around a device synchronise, upload included; the two paths alternate, --runs each after one warm-up round,
and their total_samples must be equal.  Prints one JSON line per corpus.  --paths device (or host) opens through one
path only, for a kernel trace of it.

--classes K: the range calls of an index over K header classes instead.  The files are dealt evenly over the first K
stereo mode packs of tools/bench_decode_mixed.py's CLASSES; one call decodes --ranges random windows of --window
seconds over all files:
    mixed      one OggIndex(one_decoder=True): one decode_ranges call
    per_class  K single-class OggIndex, each given its own files' windows (sorted by class beforehand, which the
               timing leaves out): K decode_ranges calls
Device events around the calls, median over --reps after a warm-up; the two must give equal got and equal PCM.
--arms per_class (or mixed) times one of them alone: per_class runs on a build without mixed range stores too."""
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


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def class_files(v, K, nfiles, seconds, signals):
    """-> (files, class of every file): nfiles files dealt over K classes, file i of class i % K"""
    from tests.signals import burst_signal
    from tools.bench_decode_mixed import CLASSES
    if not 1 <= K <= len(CLASSES) or nfiles % K:
        sys.exit(f"--classes must be 1..{len(CLASSES)} and divide --files")
    per = []
    for rate, q in CLASSES[:K]:
        n = int(seconds * rate)
        per.append(v.encode_ogg([burst_signal(2, rate, n, seed=700 + k, period=20000, level=1.0 if k % 4 else 0.05)
                                 for k in range(signals)], rate, quality=q))
    return [per[i % K][(i // K) % signals] for i in range(nfiles)], [i % K for i in range(nfiles)]


def ranges_report(v, a):
    K = a.classes
    from tools.bench_decode_mixed import CLASSES
    files, of = class_files(v, K, a.files, a.max_seconds, a.signals)
    arms = ["mixed", "per_class"] if a.arms == "both" else [a.arms]
    mine = [[i for i, c in enumerate(of) if c == k] for k in range(K)]
    mixed = v.OggIndex(files, device_demux=True, one_decoder=True, max_batch=a.max_batch) if "mixed" in arms else None
    single = [v.OggIndex([files[i] for i in m], device_demux=True, max_batch=a.max_batch) for m in mine] \
        if "per_class" in arms else []
    totals = mixed.total_samples if mixed else [int(single[c].total_samples[i // K]) for i, c in enumerate(of)]
    rng = np.random.default_rng(a.seed)
    ids = rng.integers(0, a.files, a.ranges)
    L = np.array([int(a.window * CLASSES[of[i]][0]) for i in ids])
    starts = np.array([rng.integers(0, max(1, int(totals[i]) - n)) for i, n in zip(ids, L)], np.int64)
    rows = [np.flatnonzero(np.asarray(of)[ids] == k) for k in range(K)]
    local = [np.array([mine[k].index(int(i)) for i in ids[r]], np.int64) for k, r in enumerate(rows)]
    res = {}

    def one():
        res["m"] = mixed.decode_ranges(ids, starts, L)

    def per_class():
        res["s"] = [single[k].decode_ranges(local[k], starts[r], L[r]) for k, r in enumerate(rows) if len(r)]

    fns, times = {"mixed": one, "per_class": per_class}, {arm: [] for arm in arms}
    for _ in range(a.runs):                                # the arms alternate, run by run
        for arm in arms:
            times[arm].append(statistics.median(events_ms(fns[arm], a.reps)))
    out = {"metric": "ogg_index_ranges_ms", "classes": K, "files": a.files, "seconds": a.max_seconds,
           "ranges": a.ranges, "window_seconds": a.window, "max_batch": a.max_batch, "reps": a.reps, "runs": a.runs}
    for arm in arms:
        out[arm + "_ms"], out[arm + "_ms_runs"] = statistics.median(times[arm]), times[arm]
    if len(arms) == 2:
        same, parts = True, iter(res["s"])
        for k, r in enumerate(rows):
            if len(r):
                pcm, got = next(parts)
                same &= bool(np.array_equal(got, res["m"][1][r]) and
                             torch.equal(res["m"][0][r][:, :pcm.shape[1], :pcm.shape[2]], pcm))
        out["per_class_over_mixed"], out["same_pcm"] = out["per_class_ms"] / out["mixed_ms"], same
    print(json.dumps(out), flush=True)
    for x in single + ([mixed] if mixed else []):
        x.close()


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
    ap.add_argument("--classes", type=int, default=0, help="K > 0: time range calls over K header classes instead")
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per window (--classes)")
    ap.add_argument("--max-batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--arms", choices=["both", "mixed", "per_class"], default="both")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_index.py needs a GPU: there is nothing to measure without one")
    if a.runs < 1:
        sys.exit("--runs must be at least 1")

    import vorbis_aotuv_lancer_amd as v
    from tests.signals import burst_signal

    if a.classes:
        ranges_report(v, a)
        return
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
