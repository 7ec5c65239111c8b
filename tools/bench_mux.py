#!/usr/bin/env python3
"""Ogg paging measurement (outside bench.py): vbm_ogg_mux_packets at full size on one MI355X, against the host writer.

Packets come from the device encoder as in tools/bench_decode.py: K distinct signals are encoded by the front end and
dealt round robin to `--streams` streams; every call carries one packet per stream (what one 1024-sample write of long
blocks yields) as rows [streams][max_packet_bytes] with their vbm_packet_info on the device, rows in a seeded random
order.  All inputs are built first; then `--warmup` calls run and `--steps` consecutive calls are timed with device
events, nothing but the mux calls between them.  Then the parent's way on the same packets: vbm_packets_compact, one D2H
copy of the compact run, vbm_ogg_stream_packetin + _pageout per stream on one host thread (driven through ctypes: the
cost of the same number of empty ctypes calls is measured and reported beside it).  Prints one JSON line.

Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16384)
    ap.add_argument("--signals", type=int, default=64)
    ap.add_argument("--quality", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=5, help="writes timed through the host writer")
    a = ap.parse_args()

    import vorbis_aotuv_lancer_amd as v
    from tests.signals import synth_signal

    dev = torch.device("cuda:0")
    S, K, ch, rate = a.streams, a.signals, 2, 44100
    ncalls = a.warmup + a.steps
    setup = v.Setup(ch, rate, a.quality)
    nsamp = (ncalls + 6) * 1024
    sigs = np.stack([synth_signal(ch, rate, nsamp, seed=300 + k, level=1.0 if k % 4 else 0.05) for k in range(K)])
    enc = v.Encoder(setup, K)
    M = enc.max_packet_bytes
    fe = v.FrontEnd(enc)
    lead = [[] for _ in range(K)]
    dsig = torch.from_numpy(sigs).to(dev)
    for c in range(0, nsamp, 1024):
        fe.write(dsig[:, :, c:c + 1024].contiguous())
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                break
            packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
            for r, pi in enumerate(info):
                lead[int(pi["stream"])].append((int(pi["packetno"]), bytes(packets[r, :nbytes[r]]), int(pi["granulepos"])))
    fe.close()
    enc.close()
    for x in lead:
        x.sort()
    if min(len(x) for x in lead) < ncalls:
        raise SystemExit("not enough packets per signal")

    info_dt = np.dtype(v.PacketInfo)
    rng = np.random.default_rng(9)
    lp = np.zeros((K, ncalls, M), np.uint8)
    lnb = np.zeros((K, ncalls), np.int32)
    for k in range(K):
        for t in range(ncalls):
            p = lead[k][t][1]
            lp[k, t, :len(p)] = np.frombuffer(p, np.uint8)
            lnb[k, t] = len(p)
    dlp, dlnb = torch.from_numpy(lp).to(dev), torch.from_numpy(lnb).to(dev)
    inputs = []
    for t in range(ncalls):
        order = rng.permutation(S)
        rec = np.zeros(S, info_dt)
        rec["stream"] = order
        rec["packetno"] = 3 + t
        rec["granulepos"] = np.array([lead[s % K][t][2] for s in order], np.int64)
        li = torch.from_numpy((order % K).astype(np.int64)).to(dev)
        inputs.append((torch.from_numpy(rec.view(np.uint8).reshape(S, 40).copy()).to(dev), dlp[li, t].contiguous(),
                       dlnb[li, t].contiguous(), order))
    packet_bytes = float(sum(int(x[2].sum()) for x in inputs[a.warmup:])) / a.steps

    mux = v.OggMux(setup, S, M)
    mux.start()
    for t in range(a.warmup):
        mux.mux(*inputs[t][:3])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for t in range(a.warmup, ncalls):                     # nothing but the mux calls between the events
        mux.mux(*inputs[t][:3])
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    status_bad = int((mux._ring[0][2] != 0).sum())
    # the bytes the timed calls wrote, from an untimed replay on a second mux (the ring keeps three results only)
    replay = v.OggMux(setup, S, M)
    replay.start()
    page_bytes = [int(replay.mux(*inputs[t][:3])[1][-1]) for t in range(ncalls)][a.warmup:]
    replay.close()

    # (b) the parent's way: compact, one D2H, packetin / pageout per stream on one host thread
    lib = v.lib
    hs = []
    hdrs = v.header_packets(setup)
    for s in range(S):
        h = C.c_void_p()
        v.check(lib.vbm_ogg_stream_create(C.byref(h), s), "vbm_ogg_stream_create")
        hs.append(h)
        for hp in hdrs:
            lib.vbm_ogg_stream_packetin(h, hp, len(hp), 0, 0)
        page, n = C.c_void_p(), C.c_long()
        while lib.vbm_ogg_stream_pageout(h, 1, C.byref(page), C.byref(n)) == 1:
            pass
    comp = torch.empty(S * M, dtype=torch.uint8, device=dev)
    coff = torch.empty(S + 1, dtype=torch.int64, device=dev)
    host_ms, d2h_ms, host_pages = [], [], 0
    page, n = C.c_void_p(), C.c_long()
    for t in range(min(a.host_steps, ncalls)):
        dinfo, pk, nb, order = inputs[t]
        gps = [lead[s % K][t][2] for s in order]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v.check(lib.vbm_packets_compact(pk.data_ptr(), nb.data_ptr(), S, M, comp.data_ptr(), coff.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "vbm_packets_compact")
        off = coff.cpu().numpy()
        data = comp[:int(off[-1])].cpu().numpy()
        lens = nb.cpu().numpy()
        t1 = time.perf_counter()
        base = data.ctypes.data
        for k in range(S):
            h = hs[order[k]]
            lib.vbm_ogg_stream_packetin(h, base + int(off[k]), int(lens[k]), 0, gps[k])
            while lib.vbm_ogg_stream_pageout(h, 0, C.byref(page), C.byref(n)) == 1:
                host_pages += n.value
        t2 = time.perf_counter()
        d2h_ms.append((t1 - t0) * 1e3)
        host_ms.append((t2 - t1) * 1e3)
    t0 = time.perf_counter()
    for k in range(2 * S):                                # what the ctypes calls alone cost
        lib.vbm_version()
    ctypes_ms = (time.perf_counter() - t0) * 1e3
    for h in hs:
        lib.vbm_ogg_stream_destroy(h)

    print(json.dumps({
        "metric": "ogg_mux_ms", "streams": S, "signals": K, "quality": a.quality, "steps": a.steps,
        "mux_ms_per_write": ms / a.steps, "packet_bytes_per_write": packet_bytes, "page_bytes_per_write": sum(page_bytes) / a.steps,
        "writes_with_pages": sum(1 for b in page_bytes if b),
        "status_errors": status_bad, "out_bound_bytes": mux.out_bound(S),
        "host_writer_ms_per_write": float(np.median(host_ms)) if host_ms else None,
        "host_compact_d2h_ms_per_write": float(np.median(d2h_ms)) if d2h_ms else None,
        "host_ctypes_calls_ms": ctypes_ms, "host_steps": len(host_ms),
    }))
    mux.close()


if __name__ == "__main__":
    main()
