#!/usr/bin/env python3
"""Tolerant whole-file Ogg demux measurement (outside bench.py), on one MI355X.  The corpora of tools/bench_demux.py:
    files    `--files` stereo q5 files of seeded lengths between --min-seconds and --max-seconds, made by encode_ogg
    single   one file of about --single-mb MB: packets of random bytes with the sizes of stereo q5 packets
    damaged  the files corpus with one audio page in 100 removed (resync only: the strict demux rejects those files)
For each undamaged corpus the strict scan + fill (vbm_ogg_demux_scan / _fill) and the resync scan + fill
(vbm_ogg_resync_scan / _fill) run on the same data, already on the device, in one process, alternating; the outputs of
the two are compared equal before anything is timed.  Times are device events around the work, which ends in a
synchronise, after a warm-up; medians over --reps.  Prints one JSON line per corpus: ms, GB/s of .ogg bytes, and the
resync / strict ratio.  Under rocprofv3 --kernel-trace --stats the same run gives the per-kernel times."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Strict:
    def __init__(self, v, data, off):
        from vorbis_aotuv_lancer_amd._lib import lib, check
        from vorbis_aotuv_lancer_amd.stream import FILE_INFO
        self.lib, self.check, self.data, self.off, n = lib, check, data, off, len(off) - 1
        self.h = C.c_void_p()
        check(lib.vbm_ogg_demuxer_create(C.byref(self.h), n, int(off[-1])), "vbm_ogg_demuxer_create")
        self.info = torch.zeros(n * FILE_INFO.itemsize, dtype=torch.uint8, device="cuda")
        self.totals = torch.zeros(3, dtype=torch.int64, device="cuda")
        self.q = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.scan()
        P, B, H = self.totals.cpu().tolist()
        self.sizes = (P, B, H)
        self.out = [torch.zeros(max(k, 1), dtype=d, device="cuda")
                    for k, d in ((H, torch.uint8), (B, torch.uint8), (P + 1, torch.int64), (P, torch.int64), (P, torch.uint8))]

    def scan(self):
        self.check(self.lib.vbm_ogg_demux_scan(self.h, len(self.off) - 1, self.data.data_ptr(), self.off.ctypes.data,
                                               self.info.data_ptr(), self.totals.data_ptr(), self.q), "scan")

    def fill(self):
        P, B, H = self.sizes
        h, p, o, g, e = (x.data_ptr() for x in self.out)
        self.check(self.lib.vbm_ogg_demux_fill(self.h, h, H, p, B, o, g, e, P, self.q), "fill")

    def outputs(self):
        P, B, H = self.sizes
        return [x.cpu().numpy()[:k].tobytes() for x, k in zip(self.out, (H, B, P + 1, P, P))]

    def close(self):
        self.lib.vbm_ogg_demuxer_destroy(self.h)


class Resync:
    def __init__(self, v, data, off):
        from vorbis_aotuv_lancer_amd._lib import lib, check
        from vorbis_aotuv_lancer_amd.stream import resync_meta
        self.lib, self.check, self.data, self.off, n = lib, check, data, off, len(off) - 1
        self.rd = v.ResyncDemuxer(n, int(off[-1]))
        self.cap = 2 * n + 62
        layout = resync_meta(n, self.cap)
        self.meta = torch.zeros(layout.size, dtype=torch.uint8, device="cuda")
        self.at = layout.ptrs(self.meta)
        self.q = self.rd._q()
        self.scan()
        self.totals = layout.views(self.meta.cpu().numpy())["totals"].copy()
        assert self.totals[5] == 0
        E, P, B, H = (int(x) for x in self.totals[:4])
        self.sizes = (P, B, H)
        self.out = [torch.zeros(max(k, 1), dtype=d, device="cuda")
                    for k, d in ((H, torch.uint8), (B, torch.uint8), (P + 1, torch.int64), (P, torch.int64), (P, torch.uint8),
                                 (P, torch.uint8))]

    def scan(self):
        at = self.at
        self.check(self.lib.vbm_ogg_resync_scan(self.rd._h, len(self.off) - 1, self.data.data_ptr(), self.off.ctypes.data,
                                                at["events"], at["links"], at["info"], self.cap, at["totals"], self.q), "scan")

    def fill(self):
        P, B, H = self.sizes
        h, p, o, g, e, ga = (x.data_ptr() for x in self.out)
        self.check(self.lib.vbm_ogg_resync_fill(self.rd._h, h, H, p, B, o, g, e, ga, P, self.q), "fill")

    def outputs(self):
        P, B, H = self.sizes
        return [x.cpu().numpy()[:k].tobytes() for x, k in zip(self.out, (H, B, P + 1, P, P))]

    def close(self):
        self.rd.close()


def timed(objs, reps):
    """scan and fill of every object in turn, reps + 1 rounds (the first warms up) -> per object (scan ms, fill ms)"""
    ts, tf = [[] for _ in objs], [[] for _ in objs]
    for rep in range(reps + 1):
        for k, o in enumerate(objs):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            o.scan()
            e[1].record()
            o.fill()
            e[2].record()
            torch.cuda.synchronize()
            if rep:
                ts[k].append(e[0].elapsed_time(e[1]))
                tf[k].append(e[1].elapsed_time(e[2]))
    return [(statistics.median(a), statistics.median(b)) for a, b in zip(ts, tf)]


def report(v, name, blobs, reps, strict=True):
    off = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=off[1:])
    data = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    nbytes = int(off[-1])
    objs = [Resync(v, data, off)] + ([Strict(v, data, off)] if strict else [])
    for o in objs:
        o.fill()
    same = None
    if strict:
        same = objs[0].outputs() == objs[1].outputs() and not objs[0].out[5].any().item()
        assert same, "the resync demux of undamaged files differs from the strict demux"
    times = timed(objs, reps)
    line = {"metric": "ogg_resync_demux", "corpus": name, "files": len(blobs), "ogg_bytes": nbytes,
            "entries": int(objs[0].totals[0]), "packets": int(objs[0].totals[1]), "candidates": int(objs[0].totals[4]),
            "reps": reps, "same_outputs": same}
    for o, (s, f), key in zip(objs, times, ("resync", "strict")):
        line[key] = {"scan_ms": s, "fill_ms": f, "GB_per_s": nbytes / ((s + f) / 1e3) / 1e9}
    if strict:
        line["resync_over_strict"] = {"scan": times[0][0] / times[1][0], "scan_and_fill": sum(times[0]) / sum(times[1])}
    print(json.dumps(line), flush=True)
    for o in objs:
        o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=6.0)
    ap.add_argument("--signals", type=int, default=16, help="distinct signals the files are cut from")
    ap.add_argument("--single-mb", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_demux_resync.py needs a GPU: there is nothing to measure without one")

    import vorbis_aotuv_lancer_amd as v
    from tests.ogg_pages import parse
    from tests.signals import burst_signal

    rate, rng = 44100, np.random.default_rng(a.seed)
    lengths = rng.integers(int(a.min_seconds * rate), int(a.max_seconds * rate) + 1, a.files)
    base = [burst_signal(2, rate, int(lengths.max()), seed=700 + k, period=20000, level=1.0 if k % 4 else 0.05)
            for k in range(a.signals)]
    files = v.encode_ogg([base[i % a.signals][:, :int(n)] for i, n in enumerate(lengths)], rate, quality=0.5)
    report(v, "files", files, a.reps)

    setup = v.Setup(2, rate, 0.5)
    sizes = np.clip(rng.normal(475, 150, int(a.single_mb * 1e6 / 475)), 1, 4000).astype(int)
    packets = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in sizes]
    single = v.write_ogg(setup, packets, [(1024 * (k + 1), k == len(packets) - 1) for k in range(len(packets))])
    report(v, "single", [single], a.reps)

    damaged, count = [], 0
    for f in files:                                        # every 100th audio page of the corpus goes
        out = []
        for k, p in enumerate(parse(f, 0, len(f))):
            if k >= 3:
                count += 1
                if count % 100 == 0:
                    continue
            out.append(f[p.pos:p.pos + p.size])
        damaged.append(b"".join(out))
    report(v, "damaged", damaged, a.reps, strict=False)


if __name__ == "__main__":
    main()
