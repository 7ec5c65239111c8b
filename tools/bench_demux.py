#!/usr/bin/env python3
"""Batch Ogg demux measurement (outside bench.py), on one MI355X.  Two corpora:
    files   `--files` stereo q5 files of seeded lengths between --min-seconds and --max-seconds, made by encode_ogg
    single  one file of about --single-mb MB: packets of random bytes with the sizes of stereo q5 packets, paged by
            write_ogg (the demux does not look inside a packet)
For each: vbm_ogg_demux_scan and vbm_ogg_demux_fill on data that is already on the device, timed with device events
(median over --reps after a warm-up), as GB/s of .ogg bytes; beside it demux_ogg (vbm_ogg_demux, one core) over the same
files on this machine, and the outputs of the two compared.  For the files corpus also decode_ogg end to end (wall
time around a device synchronise, upload and demux included) with device_demux off and on, alternating.  Prints one
JSON line per measurement.
--links K re-deals both corpora as chained files: the files corpus as files / K chains of K files each, the single file's
packets as one chain of K links.  The report then has the split (vbm_ogg_chain_split) in front of scan and fill, which
run over the links the split found, and decode_ogg(chained=True) end to end.  Under rocprofv3 --kernel-trace --stats
the same run puts k_chain_walk beside k_dmx_walk on the same bytes."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_demux(v, blobs, reps, chained=False):
    """-> (ms of scan, ms of fill: medians), the batch's outputs as numpy; chained: the blobs are chained files, the
    demux runs over their links, and the first of the times is the ms of the split that finds them"""
    from vorbis_aotuv_lancer_amd._lib import lib, check
    from vorbis_aotuv_lancer_amd.stream import FILE_INFO
    n = len(blobs)
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=off[1:])
    data = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    split = None
    if chained:
        sp, file_off, nfiles = v.ChainSplitter(n, int(off[-1])), off, n
        _, off = sp.split(data, file_off)                   # the demux below takes the links as its files
        n = len(off) - 1
        d_links = torch.zeros(nfiles + 1 + n + 1, dtype=torch.int64, device="cuda")

        def split():
            check(lib.vbm_ogg_chain_split(sp._h, nfiles, data.data_ptr(), file_off.ctypes.data, d_links.data_ptr(),
                                          d_links.data_ptr() + 8 * (nfiles + 1), n, sp._q()), "split")
    h = C.c_void_p()
    check(lib.vbm_ogg_demuxer_create(C.byref(h), n, int(off[-1])), "vbm_ogg_demuxer_create")
    info = torch.zeros(n * FILE_INFO.itemsize, dtype=torch.uint8, device="cuda")
    totals = torch.zeros(3, dtype=torch.int64, device="cuda")
    q = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def scan():
        check(lib.vbm_ogg_demux_scan(h, n, data.data_ptr(), off.ctypes.data, info.data_ptr(), totals.data_ptr(), q), "scan")

    scan()
    P, B, H = totals.cpu().tolist()
    hdr = torch.zeros(max(H, 1), dtype=torch.uint8, device="cuda")
    payload = torch.zeros(max(B, 1), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
    gp = torch.zeros(max(P, 1), dtype=torch.int64, device="cuda")
    eos = torch.zeros(max(P, 1), dtype=torch.uint8, device="cuda")

    def fill():
        check(lib.vbm_ogg_demux_fill(h, hdr.data_ptr(), H, payload.data_ptr(), B, offsets.data_ptr(), gp.data_ptr(),
                                     eos.data_ptr(), P, q), "fill")

    fill()
    torch.cuda.synchronize()
    tc, ts, tf = [], [], []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        if split:
            e[3].record()
            split()
        e[0].record()
        scan()
        e[1].record()
        fill()
        e[2].record()
        torch.cuda.synchronize()
        ts.append(e[0].elapsed_time(e[1]))
        tf.append(e[1].elapsed_time(e[2]))
        if split:
            tc.append(e[3].elapsed_time(e[0]))
    st = C.c_int(-1)
    check(lib.vbm_ogg_demux_status(h, C.byref(st), q), "status")
    assert st.value == 0
    out = (info.cpu().numpy().view(FILE_INFO), payload[:B].cpu().numpy(), offsets.cpu().numpy(), gp[:P].cpu().numpy(),
           eos[:P].cpu().numpy())
    lib.vbm_ogg_demuxer_destroy(h)
    if split:
        assert np.array_equal(d_links[nfiles + 1:].cpu().numpy(), off) and sp.split(data, file_off, n)[1].tolist() == off.tolist()
        sp.close()
        return statistics.median(tc), statistics.median(ts), statistics.median(tf), out
    return statistics.median(ts), statistics.median(tf), out


def host_demux(v, blobs, reps):
    """-> (seconds for all files: median), the last run's outputs"""
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = [v.demux_ogg(b) for b in blobs]
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def demux_report(v, name, blobs, reps, chains=None):
    """chains: the same links in the same order, joined into chained files"""
    nbytes = sum(len(b) for b in blobs)
    if chains:
        assert b"".join(chains) == b"".join(blobs)
        ms_split, ms_scan, ms_fill, (info, payload, offsets, gp, eos) = device_demux(v, chains, reps, chained=True)
        assert len(info) == len(blobs)
    else:
        ms_scan, ms_fill, (info, payload, offsets, gp, eos) = device_demux(v, blobs, reps)
    host_s, host = host_demux(v, blobs, max(1, min(reps, 3)))
    same = bool((info["status"] == 0).all())
    for f, (_, data, offs, g, e) in enumerate(host):
        a, at = int(info["packet_base"][f]), int(info["payload_base"][f])
        k = len(g)
        same = same and k == info["packets"][f] and np.array_equal(offsets[a:a + k + 1] - at, offs) and \
            np.array_equal(gp[a:a + k], g) and np.array_equal(eos[a:a + k], e) and \
            np.array_equal(payload[at:at + len(data)], data)
    dev_s = (ms_scan + ms_fill + (ms_split if chains else 0.0)) / 1e3
    device = {"scan_ms": ms_scan, "fill_ms": ms_fill, "GB_per_s": nbytes / dev_s / 1e9}
    if chains:
        device["split_ms"] = ms_split
    print(json.dumps({"metric": "ogg_chain_demux" if chains else "ogg_demux", "corpus": name,
                      "files": len(chains or blobs), "links": len(blobs), "ogg_bytes": nbytes,
                      "pages": int(info["pages"].sum()), "packets": int(info["packets"].sum()), "reps": reps,
                      "device": device,
                      "host_demux_ogg": {"wall_s": host_s, "GB_per_s": nbytes / host_s / 1e9},
                      "speedup": host_s / dev_s, "same_outputs": same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=6.0)
    ap.add_argument("--signals", type=int, default=16, help="distinct signals the files are cut from")
    ap.add_argument("--single-mb", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--decode-reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--links", type=int, default=0, help="K > 0: both corpora as chained files of K links")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_demux.py needs a GPU: there is nothing to measure without one")

    import vorbis_aotuv_lancer_amd as v
    from tests.signals import burst_signal

    rate, rng = 44100, np.random.default_rng(a.seed)
    lengths = rng.integers(int(a.min_seconds * rate), int(a.max_seconds * rate) + 1, a.files)
    base = [burst_signal(2, rate, int(lengths.max()), seed=700 + k, period=20000, level=1.0 if k % 4 else 0.05)
            for k in range(a.signals)]
    files = v.encode_ogg([base[i % a.signals][:, :int(n)] for i, n in enumerate(lengths)], rate, quality=0.5)
    K = a.links
    if K > 0 and a.files % K:
        sys.exit("--links must divide --files")
    chains = [b"".join(files[i:i + K]) for i in range(0, a.files, K)] if K > 0 else None
    demux_report(v, "files", files, a.reps, chains)

    setup = v.Setup(2, rate, 0.5)
    sizes = np.clip(rng.normal(475, 150, int(a.single_mb * 1e6 / 475)), 1, 4000).astype(int)
    packets = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in sizes]
    if K > 0:
        per = (len(packets) + K - 1) // K
        parts = [packets[i:i + per] for i in range(0, len(packets), per)]
        links = [v.write_ogg(setup, p, [(1024 * (k + 1), k == len(p) - 1) for k in range(len(p))], serialno=1 + i)
                 for i, p in enumerate(parts)]
        demux_report(v, "single", links, a.reps, [b"".join(links)])
    else:
        single = v.write_ogg(setup, packets, [(1024 * (k + 1), k == len(packets) - 1) for k in range(len(packets))])
        demux_report(v, "single", [single], a.reps)

    if a.decode_reps <= 0:
        return
    # decode_ogg end to end, host demux and device demux alternating
    times = {False: [], True: []}
    outs = {}
    for rep in range(a.decode_reps + 1):                   # the first round warms up
        for dd in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[dd] = v.decode_ogg(chains, device_demux=dd, chained=True) if chains else v.decode_ogg(files, device_demux=dd)
            torch.cuda.synchronize()
            if rep:
                times[dd].append(time.perf_counter() - t0)
    if chains:
        outs = {dd: [link for per_file in outs[dd] for link in per_file] for dd in outs}
        assert len(outs[True]) == a.files
    same = all(torch.equal(x[0], y[0]) for x, y in zip(outs[False], outs[True]))
    audio_s = float(lengths.sum()) / rate
    t_off, t_on = statistics.median(times[False]), statistics.median(times[True])
    print(json.dumps({"metric": "decode_ogg_end_to_end", "files": len(chains or files), "links": a.files,
                      "chained": bool(chains), "audio_seconds": audio_s,
                      "ogg_bytes": sum(len(f) for f in files), "reps": a.decode_reps,
                      "device_demux_off": {"wall_s": t_off, "runs_s": times[False], "audio_s_per_s": audio_s / t_off},
                      "device_demux_on": {"wall_s": t_on, "runs_s": times[True], "audio_s_per_s": audio_s / t_on},
                      "speedup": t_off / t_on, "same_pcm": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
