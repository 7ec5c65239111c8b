#!/usr/bin/env python3
"""Incremental Ogg demux measurement (outside bench.py), on one MI355X: vbm_ogg_feed_scan / _fill for `--streams` live
stereo q5 streams.

The streams come from the device encoder and OggMux: `--signals` distinct signals are encoded for `--writes` writes of
1024 samples, paged by OggMux, and dealt round robin to the slots.  A stream's bytes (header pages, then audio pages)
are cut into `--writes` equal pieces, the bytes one write produces on average, and call t gives every slot its piece t:
pages are about nine pieces long, so nearly every call starts and ends inside a page.  All inputs are on the device
before anything is timed.  One pass through OggFeed.push checks the outputs against demux_ogg; then the slots are reset
and the same calls run `--reps` + 1 times (the first warms up) with device events around every scan and every fill.
Reported: the medians over the passes of the mean scan and fill time per call, GB/s of .ogg bytes, packets per call; and
on the same bytes demux_ogg on one core (median of 3) and the batch demux (vbm_ogg_demux_scan / _fill) given the same
streams whole.  Prints one JSON line.

Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def make_streams(v, K, writes, quality):
    """-> K byte runs: the header pages and the pages OggMux makes of `writes` writes of the device encoder"""
    from tests.signals import synth_signal
    dev = torch.device("cuda:0")
    ch, rate = 2, 44100
    setup = v.Setup(ch, rate, quality)
    nsamp = writes * 1024
    sigs = np.stack([synth_signal(ch, rate, nsamp, seed=300 + k, level=1.0 if k % 4 else 0.05) for k in range(K)])
    enc = v.Encoder(setup, K)
    fe = v.FrontEnd(enc)
    mux = v.OggMux(setup, K, enc.max_packet_bytes)
    runs = [bytearray(h) for h in mux.start()]
    dsig = torch.from_numpy(sigs).to(dev)
    for c in range(0, nsamp, 1024):
        fe.write(dsig[:, :, c:c + 1024].contiguous())
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                break
            out, offsets, status = mux.mux(info, packets, nbytes, flush=c + 1024 >= nsamp)
            off = offsets.cpu().numpy()
            assert not status.cpu().numpy().any()
            raw = out[:int(off[-1])].cpu().numpy().tobytes()
            for k in range(K):
                runs[k] += raw[off[k]:off[k + 1]]
    mux.close()
    fe.close()
    enc.close()
    return [bytes(r) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--quality", type=float, default=0.5)
    ap.add_argument("--writes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--max-page-carry", type=int, default=8192)
    ap.add_argument("--max-packet-bytes", type=int, default=8192)
    ap.add_argument("--header-cap", type=int, default=8192)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_feed.py needs a GPU: there is nothing to measure without one")

    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib, check
    from vorbis_aotuv_lancer_amd.stream import FEED_INFO
    from bench_demux import device_demux

    S, K, T = a.streams, a.signals, a.writes
    runs = make_streams(v, K, T, a.quality)
    piece = [-(-len(r) // T) for r in runs]
    ids = np.arange(S, dtype=np.int32)
    calls = []
    for t in range(T):
        parts = [runs[k][t * piece[k]:(t + 1) * piece[k]] for k in range(K)]
        off = np.zeros(S + 1, np.int64)
        np.cumsum([len(parts[s % K]) for s in range(S)], out=off[1:])
        data = torch.from_numpy(np.frombuffer(b"".join(parts[s % K] for s in range(S)), np.uint8).copy()).cuda()
        end = np.full(S, t == T - 1, np.uint8)
        calls.append((data, off, end))
    call_bytes = [int(c[1][-1]) for c in calls]
    total_bytes = sum(call_bytes)

    # one pass through the class: the outputs against demux_ogg
    feed = v.OggFeed(S, max(call_bytes), max_page_carry=a.max_page_carry, max_packet_bytes=a.max_packet_bytes,
                     header_cap=a.header_cap)
    want = [v.demux_ogg(r) for r in runs]
    check_slots = sorted(set(range(min(K, S))) | set(range(max(0, S - K), S)))
    acc = {s: dict(payload=[], sizes=[], gp=[], eos=[]) for s in check_slots}
    caps, packets_per_call, status_bad = [], [], 0
    for data, off, end in calls:
        r = feed.push(ids, data, end=end, offsets=off)
        caps.append((int(r.offsets.numel()) - 1, int(r.payload.numel())))
        packets_per_call.append(caps[-1][0])
        status_bad += int(np.count_nonzero(r.info["status"]))
        offs, pay, gp, eos = r.offsets.cpu().numpy(), r.payload.cpu().numpy(), r.granulepos.cpu().numpy(), r.eos.cpu().numpy()
        for s in check_slots:
            p, n = int(r.info["packet_base"][s]), int(r.info["packets"][s])
            acc[s]["payload"].append(pay[offs[p]:offs[p + n]].tobytes())
            acc[s]["sizes"] += np.diff(offs[p:p + n + 1]).tolist()
            acc[s]["gp"] += gp[p:p + n].tolist()
            acc[s]["eos"] += eos[p:p + n].tolist()
    same = status_bad == 0
    for s in check_slots:
        h, body, offs, gp, eos = want[s % K]
        same = same and feed.headers(s) == h and b"".join(acc[s]["payload"]) == body.tobytes() and \
            acc[s]["sizes"] == np.diff(offs).tolist() and acc[s]["gp"] == gp.tolist() and acc[s]["eos"] == eos.tolist()
    same = same and sum(packets_per_call) == sum(len(want[s % K][3]) for s in range(S))

    # the timed passes: raw calls, outputs of the sizes the first pass found, device events around every scan and fill
    q = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    meta = torch.zeros(16 + S * FEED_INFO.itemsize, dtype=torch.uint8, device="cuda")
    P, B = max(c[0] for c in caps), max(c[1] for c in caps)
    payload = torch.zeros(max(B, 1), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
    gp = torch.zeros(max(P, 1), dtype=torch.int64, device="cuda")
    eos = torch.zeros(max(P, 1), dtype=torch.uint8, device="cuda")
    scan_ms, fill_ms = [], []
    for rep in range(a.reps + 1):
        feed.reset(ids)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in calls]
        for (data, off, end), e, (cp, cb) in zip(calls, ev, caps):
            e[0].record()
            check(lib.vbm_ogg_feed_scan(feed._h, S, ids.ctypes.data, data.data_ptr(), off.ctypes.data, end.ctypes.data,
                                        meta.data_ptr() + 16, meta.data_ptr(), q), "vbm_ogg_feed_scan")
            e[1].record()
            check(lib.vbm_ogg_feed_fill(feed._h, payload.data_ptr(), cb, offsets.data_ptr(), gp.data_ptr(), eos.data_ptr(), cp,
                                        q), "vbm_ogg_feed_fill")
            e[2].record()
        torch.cuda.synchronize()
        st = C.c_int(-1)
        check(lib.vbm_ogg_feed_status(feed._h, C.byref(st), q), "vbm_ogg_feed_status")
        assert st.value == 0, st.value
        if rep:
            scan_ms.append(statistics.mean(e[0].elapsed_time(e[1]) for e in ev))
            fill_ms.append(statistics.mean(e[1].elapsed_time(e[2]) for e in ev))
    feed.close()
    ms_scan, ms_fill = statistics.median(scan_ms), statistics.median(fill_ms)

    # the same bytes as whole files: demux_ogg on one core, and the batch demux on the device
    files = [runs[s % K] for s in range(S)]
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for f in files:
            v.demux_ogg(f)
        host.append(time.perf_counter() - t0)
    host_s = statistics.median(host)
    b_scan, b_fill, _ = device_demux(v, files, a.reps)

    per_call = total_bytes / T
    state = 72 + a.max_page_carry + a.max_packet_bytes + a.header_cap
    print(json.dumps({
        "metric": "ogg_feed", "streams": S, "signals": K, "quality": a.quality, "calls": T, "reps": a.reps,
        "ogg_bytes_per_call": per_call, "bytes_per_stream_per_call": per_call / S,
        "packets_per_call": statistics.mean(packets_per_call), "same_outputs": bool(same),
        "feed": {"scan_ms": ms_scan, "fill_ms": ms_fill, "GB_per_s": per_call / ((ms_scan + ms_fill) / 1e3) / 1e9,
                 "ms_for_all_calls": (ms_scan + ms_fill) * T},
        "host_demux_ogg": {"wall_s": host_s, "GB_per_s": total_bytes / host_s / 1e9},
        "batch_demux_whole_files": {"scan_ms": b_scan, "fill_ms": b_fill,
                                    "GB_per_s": total_bytes / ((b_scan + b_fill) / 1e3) / 1e9},
        "state_bytes_per_slot": state, "state_MiB": state * S / 2 ** 20,
        "capacities": {"max_page_carry": a.max_page_carry, "max_packet_bytes": a.max_packet_bytes, "header_cap": a.header_cap},
    }), flush=True)


if __name__ == "__main__":
    main()
