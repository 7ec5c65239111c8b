#!/usr/bin/env python3
"""Ogg cut measurement (outside bench.py), on one MI355X.  Prints one JSON line.

`--files` stereo q5 files of `--seconds` seconds (encode_ogg of `--signals` distinct signals, each file one of them again
under its own serial number) are opened as an OggIndex through the device demux.  One call cuts `--ranges` random
windows of `--window` seconds, every one its own output file:
    cut        vbm_ogg_cut_ranges into a buffer of exactly the outputs' size, device events around the call
               (upload of the records and header pages, both plan runs, the scan, the emit), median over --reps after a
               warm-up
    plan_only  the same call with out_cap = 0 (the sizing call): upload, one plan run, the scan
    copy       a device-to-device copy_ of as many bytes as the cut writes: the floor of the emit, which reads and
               writes every output byte once
    host_twin  vbm_host_ogg_cut_ranges of the same call on one core over the same index in host memory (wall time,
               median of --host-reps): what a user can do today without a re-encode
    host_prep  the wall time of making the files' header pages with the host writer (one OggStream per file; the cut
               writes each output's serial number into them), which OggIndex.cut_ranges spends once; not part of `cut`
The device's outputs are compared with the twin's byte for byte.

--classes K: the files are dealt evenly over K header classes (tools/bench_index.py's class_files) and one call of
OggIndex(one_decoder=True).cut_ranges(out=) over all windows is timed against K single-class indexes, each given its
own files' windows (sorted by class beforehand, outside the timing): cut_ms of both, and the clips must be equal.
--arms per_class times the single-class indexes alone: that runs on a build without mixed range stores too."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events_ms(torch, fn, reps):
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


def classes_report(v, torch, a):
    from tools.bench_decode_mixed import CLASSES
    from tools.bench_index import class_files
    K = a.classes
    files, of = class_files(v, K, a.files, a.seconds, a.signals)
    arms = ["mixed", "per_class"] if a.arms == "both" else [a.arms]
    mine = [[i for i, c in enumerate(of) if c == k] for k in range(K)]
    mixed = v.OggIndex(files, device_demux=True, one_decoder=True) if "mixed" in arms else None
    single = [v.OggIndex([files[i] for i in m], device_demux=True) for m in mine]
    totals = [int(single[c].total_samples[i // K]) for i, c in enumerate(of)]
    rng = np.random.default_rng(a.seed)
    ids = rng.integers(0, a.files, a.ranges)
    L = np.array([int(a.window * CLASSES[of[i]][0]) for i in ids], np.int64)
    starts = np.array([rng.integers(0, max(1, totals[i] - n)) for i, n in zip(ids, L)], np.int64)
    serials = np.arange(a.ranges)
    rows = [np.flatnonzero(np.asarray(of)[ids] == k) for k in range(K)]
    local = [np.array([mine[k].index(int(i)) for i in ids[r]], np.int64) for k, r in enumerate(rows)]
    clips = [None] * a.ranges                                          # the list form: the sizes, and the reference
    for k, r in enumerate(rows):
        for i, c in zip(r, single[k].cut_ranges(local[k], starts[r], L[r], serials[r])[0]):
            clips[i] = c
    size = np.array([len(c) for c in clips])
    out = torch.zeros(int(size.sum()), dtype=torch.uint8, device="cuda")
    outs = [torch.zeros(int(size[r].sum()), dtype=torch.uint8, device="cuda") for r in rows]
    res = {}

    def one():
        res["m"] = mixed.cut_ranges(ids, starts, L, serials, out=out)

    def per_class():
        res["s"] = [single[k].cut_ranges(local[k], starts[r], L[r], serials[r], out=outs[k])
                    for k, r in enumerate(rows) if len(r)]

    fns, times = {"mixed": one, "per_class": per_class}, {arm: [] for arm in arms}
    for _ in range(a.runs):                                            # the arms alternate, run by run
        for arm in arms:
            times[arm].append(statistics.median(events_ms(torch, fns[arm], a.reps)))
    same = mixed is None or out.cpu().numpy().tobytes() == b"".join(clips)
    for k, r in enumerate(rows):
        same &= outs[k].cpu().numpy().tobytes() == b"".join(clips[i] for i in r)
    res = {"metric": "ogg_cut_classes_ms", "classes": K, "files": a.files, "seconds": a.seconds, "ranges": a.ranges,
           "window_seconds": a.window, "out_bytes": int(size.sum()), "reps": a.reps, "runs": a.runs,
           "same_outputs": bool(same)}
    for arm in arms:
        res[arm + "_ms"], res[arm + "_ms_runs"] = statistics.median(times[arm]), times[arm]
    if len(arms) == 2:
        res["per_class_over_mixed"] = res["per_class_ms"] / res["mixed_ms"]
    print(json.dumps(res), flush=True)
    for x in single + ([mixed] if mixed else []):
        x.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--signals", type=int, default=16, help="distinct signals the files are encoded from")
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--window", type=float, default=5.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--classes", type=int, default=0, help="K > 0: one mixed index against K single-class ones")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--arms", choices=["both", "per_class"], default="both")
    a = ap.parse_args()

    import torch
    import vorbis_aotuv_lancer_amd as v
    from tests.signals import burst_signal

    if a.classes:
        classes_report(v, torch, a)
        return
    rate, n = 44100, int(a.seconds * 44100)
    base = v.encode_ogg([burst_signal(2, rate, n, seed=900 + k, period=20000, level=1.0 if k % 4 else 0.05)
                         for k in range(a.signals)], rate, quality=0.5)
    files = [base[i % a.signals] for i in range(a.files)]
    idx = v.OggIndex(files, device_demux=True)
    rng = np.random.default_rng(a.seed)
    L = int(a.window * rate)
    ids = rng.integers(0, a.files, a.ranges)
    starts = np.array([rng.integers(0, max(1, int(idx.total_samples[i]) - L)) for i in ids], np.int64)
    lengths = np.full(a.ranges, L, np.int64)
    serials = np.arange(a.ranges)

    t0 = time.perf_counter()
    per_file = [v.header_pages(h, 0) for h in idx.headers]      # what OggIndex.cut_ranges makes, once per file
    pages = [per_file[int(i)] for i in ids]
    host_prep = time.perf_counter() - t0
    hb = sum(len(p) for p in set(pages))

    sizer = v.OggCutter(a.ranges, 0, hb)
    off = sizer.cut(idx.store, ids, starts, lengths, pages, serials)[0]
    total = int(off[-1].item())
    sizer.close()
    cutter = v.OggCutter(a.ranges, total, hb)
    out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    src, ref = torch.zeros_like(out), torch.zeros_like(out)
    res = {}

    def cut(buf):
        res["r"] = cutter.cut(idx.store, ids, starts, lengths, pages, serials, out=buf)

    whole = events_ms(torch, lambda: cut(out), a.reps)
    d_off, d_stat = res["r"][0].cpu().numpy(), res["r"][1].cpu().numpy()
    plan = events_ms(torch, lambda: cut(None), a.reps)
    copy = events_ms(torch, lambda: ref.copy_(src), a.reps)

    # the host twin over the same index: the distinct files demuxed and indexed on the host, laid out as the store is
    ds = v.DecodeSetup(idx.headers[0])
    parts = []
    for blob in base:
        _, data, offsets, gp, eos = v.demux_ogg(blob)
        status, begin, end, out_start, totals = v.decode_index_scan_host(ds, data, offsets, gp, eos)
        parts.append((data, offsets, status, begin, out_start + (end - begin), int(totals[0])))
    ds.close()
    per = [parts[i % a.signals] for i in range(a.files)]
    first = np.cumsum([0] + [len(p[1]) - 1 for p in per]).astype(np.int64)
    bases = np.cumsum([0] + [len(p[0]) for p in per])
    index = (first, np.concatenate([p[2] for p in per]), np.concatenate([p[3] for p in per]),
             np.concatenate([p[4] for p in per]), np.array([p[5] for p in per], np.int64),
             np.concatenate([p[0] for p in per]),
             np.concatenate([np.zeros(1, np.int64)] + [p[1][1:] + b for p, b in zip(per, bases)]))
    twin = v.OggCutter(a.ranges, total, hb, host=True)
    h_out = np.zeros(total, np.uint8)
    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        h_off, h_stat, _, _ = twin.cut(index, ids, starts, lengths, pages, serials, out=h_out)
        host.append(time.perf_counter() - t0)
    twin.close()
    same = bool(np.array_equal(h_off, d_off) and np.array_equal(h_stat, d_stat) and
                np.array_equal(out.cpu().numpy(), h_out))
    cutter.close()
    idx.close()

    w, p, c, h = (statistics.median(x) for x in (whole, plan, copy, host))
    print(json.dumps({"metric": "ogg_cut", "files": a.files, "seconds": a.seconds, "distinct_files": a.signals,
                      "ranges": a.ranges, "window_seconds": a.window, "store_bytes": int(bases[-1]), "out_bytes": total,
                      "header_bytes": hb, "refused": int((d_stat[:-1] != 0).sum()), "status_word": int(d_stat[-1]),
                      "reps": a.reps, "cut_ms": w, "plan_only_ms": p, "copy_ms": c, "host_twin_s": h,
                      "host_prep_s": host_prep, "cut_GB_per_s_written": total / w / 1e6,
                      "copy_GB_per_s_written": total / c / 1e6, "cut_over_copy": w / c,
                      "host_twin_over_cut": h * 1e3 / w, "same_outputs": same, "cut_ms_series": whole,
                      "plan_only_ms_series": plan, "copy_ms_series": copy, "host_twin_s_series": host}), flush=True)


if __name__ == "__main__":
    main()
