#!/usr/bin/env python3
"""Ogg stream selection measurement (outside bench.py), on one MI355X.  Prints one JSON line per measurement.
    plain   `--files` stereo q5 files made by encode_ogg, repeated until they fill --plain-mb MB: everything is kept, one
            run per file.  vbm_ogg_select on data that is already on the device, timed with device events (median over
            --reps after a warm-up), beside a device-to-device copy_ of the same bytes, the yardstick of k_sel_copy.
            The walk alone is the same call with out_cap = 0: the status becomes VBM_OGG_DEMUX_ECAP and every block of
            the copy kernel exits at once, so what is left is the upload of the offsets, k_sel_walk, k_sel_scan and an
            empty launch.  Ratios to the copy_: of the whole call, and of the call less the walk.
    muxed   the same `--files` files, each with a video-like foreign stream of --video-ratio times its bytes between its
            pages (pages of 64 segments of 255 bytes; their CRC field is 0: nothing on this path reads it).
            demux_ogg_device(multiplexed=True) end to end (wall time around a device synchronise, upload included),
            beside demux_ogg_device of the Vorbis-only files, and the host alternative: select_vorbis_stream per file,
            then demux_ogg_device of what it returns; and the upload of the multiplexed files alone (the join and the one
            H2D copy that demux_ogg_device starts with).  The four alternate; the outputs are compared.
--baseline-only times demux_ogg_device of the Vorbis-only files alone and uses nothing this tool's subject added, so
that with --root it runs on an older tree (the parent commit, built) for the comparison across commits."""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np


def page_lengths(blob):
    out, pos = [], 0
    while pos < len(blob):
        nseg = blob[pos + 26]
        n = 27 + nseg + sum(blob[pos + 27:pos + 27 + nseg])
        out.append(n)
        pos += n
    return out


def mux(blob, ratio, serial, rng):
    """the pages of `blob` with a foreign stream of about ratio * len(blob) bytes between them, its head page first"""
    head = b"OggS\0\2" + struct.pack("<qIII", 0, serial, 0, 0) + b"\1\x2a" + b"\x80theora" + bytes(35)
    body = rng.integers(0, 256, 64 * 255, dtype=np.uint8).tobytes()
    lens = page_lengths(blob)
    per_gap = ratio * len(blob) / (27 + 64 + len(body)) / max(1, len(lens) - 1)
    out, pos, seq, owed = [head], 0, 1, 0.0
    for k, n in enumerate(lens):
        out.append(blob[pos:pos + n])
        pos += n
        if k < len(lens) - 1:
            owed += per_gap
            while owed >= 1:
                out.append(b"OggS\0\0" + struct.pack("<qIII", seq, serial, seq, 0) + b"\x40" + b"\xff" * 64 + body)
                seq += 1
                owed -= 1
    return b"".join(out)


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


def plain_report(v, torch, files, plain_mb, reps):
    from vorbis_aotuv_lancer_amd._lib import lib, check
    from vorbis_aotuv_lancer_amd.stream import select_meta
    per = sum(len(f) for f in files)
    blobs = files * max(1, int(plain_mb * 1e6 / per))
    n = len(blobs)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=off[1:])
    nbytes = int(off[-1])
    data = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    out, ref = torch.zeros_like(data), torch.zeros_like(data)
    layout = select_meta(n)
    meta = torch.zeros(layout.size, dtype=torch.uint8, device="cuda")
    at = layout.ptrs(meta)
    sel = v.StreamSelector(n, nbytes)

    def call(cap):
        check(lib.vbm_ogg_select(sel._h, n, data.data_ptr(), off.ctypes.data, out.data_ptr(), cap, at["out_off"], at["info"],
                                 sel._q()), "vbm_ogg_select")

    whole = events_ms(torch, lambda: call(nbytes), reps)
    same = bool(torch.equal(out, data)) and np.array_equal(layout.views(meta.cpu().numpy())["out_off"], off)
    walk = events_ms(torch, lambda: call(0), reps)
    copy = events_ms(torch, lambda: ref.copy_(data), reps)
    sel.close()
    w, k, c = statistics.median(whole), statistics.median(walk), statistics.median(copy)
    print(json.dumps({"metric": "ogg_select_plain", "files": n, "ogg_bytes": nbytes, "reps": reps,
                      "select_ms": w, "walk_only_ms": k, "copy_ms": c,
                      "select_GB_per_s_read_and_written": 2 * nbytes / w / 1e6, "copy_GB_per_s_read_and_written": 2 * nbytes / c / 1e6,
                      "ratio_with_walk": w / c, "ratio_without_walk": (w - k) / c, "same_outputs": same,
                      "select_ms_series": whole, "walk_only_ms_series": walk, "copy_ms_series": copy}), flush=True)


def wall(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def muxed_report(v, torch, files, muxed, reps, baseline_only):
    from vorbis_aotuv_lancer_amd._twin import Mem
    mem = Mem(torch.device("cuda", torch.cuda.current_device()))
    ways = {"vorbis_only": lambda: v.demux_ogg_device(files)}
    if not baseline_only:
        ways["multiplexed"] = lambda: v.demux_ogg_device(muxed, multiplexed=True)
        ways["host_select_then_upload"] = lambda: v.demux_ogg_device([v.select_vorbis_stream(m) for m in muxed])
        ways["upload_alone"] = lambda: mem.join(muxed)       # what multiplexed=True spends before its first kernel
    times, outs = {w: [] for w in ways}, {}
    for rep in range(reps + 1):                            # the first round warms up
        for w, fn in ways.items():
            t, outs[w] = wall(torch, fn)
            if rep:
                times[w].append(t)
    ref = outs["vorbis_only"]
    outs.pop("upload_alone", None)
    same = all(o.status == ref.status and o.headers == ref.headers and torch.equal(o.payload, ref.payload)
               and torch.equal(o.offsets, ref.offsets) and torch.equal(o.granulepos, ref.granulepos)
               and torch.equal(o.eos, ref.eos) for o in outs.values()) and not any(ref.status)
    rec = {"metric": "ogg_select_muxed", "files": len(files), "vorbis_bytes": sum(len(f) for f in files),
           "muxed_bytes": sum(len(m) for m in muxed), "reps": reps, "same_outputs": bool(same)}
    for w in ways:
        rec[w] = {"wall_s": statistics.median(times[w]), "runs_s": times[w]}
    if not baseline_only:
        rec["multiplexed_over_vorbis_only"] = rec["multiplexed"]["wall_s"] / rec["vorbis_only"]["wall_s"]
        rec["host_alternative_over_multiplexed"] = rec["host_select_then_upload"]["wall_s"] / rec["multiplexed"]["wall_s"]
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the built tree to import the package from")
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=6.0)
    ap.add_argument("--signals", type=int, default=16, help="distinct signals the files are cut from")
    ap.add_argument("--plain-mb", type=float, default=256.0)
    ap.add_argument("--video-ratio", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_select.py needs a GPU: there is nothing to measure without one")
    import vorbis_aotuv_lancer_amd as v
    from tests.signals import burst_signal

    rate, rng = 44100, np.random.default_rng(a.seed)
    lengths = rng.integers(int(a.min_seconds * rate), int(a.max_seconds * rate) + 1, a.files)
    base = [burst_signal(2, rate, int(lengths.max()), seed=700 + k, period=20000, level=1.0 if k % 4 else 0.05)
            for k in range(a.signals)]
    files = v.encode_ogg([base[i % a.signals][:, :int(n)] for i, n in enumerate(lengths)], rate, quality=0.5)
    if not a.baseline_only:
        plain_report(v, torch, files, a.plain_mb, a.reps)
    muxed = [mux(f, a.video_ratio, 900000 + i, rng) for i, f in enumerate(files)]
    muxed_report(v, torch, files, muxed, a.reps, a.baseline_only)


if __name__ == "__main__":
    main()
