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

`--resync` runs the same calls through a resync feed (vbm_ogg_feed_create2 with VBM_OGG_FEED_RESYNC; scan, scan_events,
fill_gaps).  Before anything is timed every call's outputs are compared with the strict feed's; then the same passes are
timed, and once more on streams that have lost pages (four copies of every signal, every audio page of a copy lost
with probability 1/100, seeded; `--lose` sets the rate), where the first pass counts the gap marks and the bytes calls
gave back.  The whole-file
comparisons are left out.

`--multiplexed [--foreign-ratio K]` (with or without `--resync`) measures a feed made with multiplexed=True on the same
mounts with a video-like foreign stream of K times their bytes between their pages (a foreign head page in front of the
Vorbis one, then behind every audio page foreign pages of up to 4096 bytes, K times the page's bytes in all), cut into
the same number of calls.  The first pass compares the packets of every slot with demux_ogg of the Vorbis-only mount;
then the same timed passes.  Reported beside the unflagged feed of the same kind on the Vorbis-only mounts, and the
flagged feed on the Vorbis-only mounts.  The whole-file comparisons are left out.

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


def cut_calls(runs, S, T):
    """call t gives slot s piece t of runs[s % K] -> [(data on the device, offsets, end)]"""
    K = len(runs)
    piece = [-(-len(r) // T) for r in runs]
    calls = []
    for t in range(T):
        parts = [runs[k][t * piece[k]:(t + 1) * piece[k]] for k in range(K)]
        off = np.zeros(S + 1, np.int64)
        np.cumsum([len(parts[s % K]) for s in range(S)], out=off[1:])
        data = torch.from_numpy(np.frombuffer(b"".join(parts[s % K] for s in range(S)), np.uint8).copy()).cuda()
        calls.append((data, off, np.full(S, t == T - 1, np.uint8)))
    return calls


def _ends(pages):
    """packets that end on these pages"""
    return sum(1 for p in pages for lv in p[27:27 + p[26]] if lv < 255)


def lose_pages(runs, rate, seed=1):
    """every page behind those of the three header packets goes with probability `rate` -> (runs, pages lost)"""
    rng, out, lost = np.random.default_rng(seed), [], 0
    for r in runs:
        pages, at = [], 0
        while at < len(r):
            n = 27 + r[at + 26] + sum(r[at + 27:at + 27 + r[at + 26]])
            pages.append(r[at:at + n])
            at += n
        headers = next(k + 1 for k in range(len(pages)) if _ends(pages[:k + 1]) >= 3)
        keep = [p for k, p in enumerate(pages) if k < headers or rng.random() >= rate]
        lost += len(pages) - len(keep)
        out.append(b"".join(keep))
    return out, lost


def multiplex(runs, ratio, seed=5):
    """every run with a foreign stream of `ratio` times its bytes between its pages -> (runs, foreign pages per run)"""
    from tests.ogg_select_cases import sized_page
    rng, out, counts = np.random.default_rng(seed), [], []
    for k, r in enumerate(runs):
        serial, seq, at, parts, owed = 0x7e000000 + k, 1, 0, [sized_page(0x7e000000 + k, 0, 27 + 1 + 42, rng, flags=2)], 0.0
        while at < len(r):
            n = 27 + r[at + 26] + sum(r[at + 27:at + 27 + r[at + 26]])
            parts.append(r[at:at + n])
            at += n
            owed += ratio * n
            while at > n and owed >= 27:                            # behind the Vorbis head page
                take = int(min(owed, 4096))
                parts.append(sized_page(serial, seq, take, rng))
                seq, owed = seq + 1, owed - take
        out.append(b"".join(parts))
        counts.append(seq)
    return out, counts


def multiplexed_run(v, lib, check, a, runs, ids, want):
    """--multiplexed: a flagged feed on the multiplexed mounts (outputs against demux_ogg of the Vorbis-only mounts,
    then the timed passes), and on the Vorbis-only mounts -> the JSON fields"""
    S, K, T = a.streams, len(runs), a.writes
    kw = dict(max_page_carry=a.max_page_carry, max_packet_bytes=a.max_packet_bytes, header_cap=a.header_cap,
              resync=a.resync, multiplexed=True)
    out = {}
    muxed, nforeign = multiplex(runs, a.foreign_ratio)
    for name, mounts in (("multiplexed_mounts", muxed), ("vorbis_only_mounts", runs)):
        calls = cut_calls(mounts, S, T)
        feed = v.OggFeed(S, max(int(c[1][-1]) for c in calls), **kw)
        caps, packets, ignored = [], np.zeros(S, np.int64), 0
        body = [[] for _ in range(min(K, S))]
        for data, off, end in calls:
            r = feed.push(ids, data, end=end, offsets=off)
            assert not r.info["status"].any() and (r.left is None or not r.left.any())
            caps.append((int(r.offsets.numel()) - 1, int(r.payload.numel())))
            packets += r.counts
            ignored += int(r.events["ignored_pages"].sum()) if a.resync else 0
            offs, pay = r.offsets.cpu().numpy(), r.payload.cpu().numpy()
            for s in range(len(body)):
                p, n = int(r.info["packet_base"][s]), int(r.info["packets"][s])
                body[s].append(pay[offs[p]:offs[p + n]].tobytes())
        same = all(packets[s] == len(want[s % K][3]) for s in range(S)) and \
            all(b"".join(body[s]) == want[s][1].tobytes() and feed.headers(s) == want[s][0] for s in range(len(body)))
        if a.resync:
            same = same and ignored == (sum(nforeign[s % K] for s in range(S)) if mounts is muxed else 0)
        scan, fill = timed_passes(lib, check, feed, ids, calls, caps, a.reps, a.resync)
        feed.close()
        per_call = sum(int(c[1][-1]) for c in calls) / T
        out[name] = {"same_packets_as_demux_ogg": bool(same), "bytes_per_call": per_call, "scan_ms": scan, "fill_ms": fill,
                     "ms_per_push": scan + fill, "GB_per_s": per_call / ((scan + fill) / 1e3) / 1e9}
    out["foreign_ratio"] = a.foreign_ratio
    out["foreign_pages_per_call"] = sum(nforeign[s % K] for s in range(S)) / T
    return out


def timed_passes(lib, check, feed, ids, calls, caps, reps, resync):
    """the calls reps + 1 times from fresh slots (the first pass warms up), device events around every scan and every
    fill -> the medians over the passes of the mean scan and fill time per call, in ms"""
    from vorbis_aotuv_lancer_amd.stream import FEED_EVENTS, FEED_INFO
    S = len(ids)
    q = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    meta = torch.zeros(16 + S * (FEED_INFO.itemsize + FEED_EVENTS.itemsize), dtype=torch.uint8, device="cuda")
    P, B = max(c[0] for c in caps), max(c[1] for c in caps)
    payload = torch.zeros(max(B, 1), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(P + 1, dtype=torch.int64, device="cuda")
    gp = torch.zeros(max(P, 1), dtype=torch.int64, device="cuda")
    eos = torch.zeros(max(P, 1), dtype=torch.uint8, device="cuda")
    gap = torch.zeros(max(P, 1), dtype=torch.uint8, device="cuda")
    scan_ms, fill_ms = [], []
    for rep in range(reps + 1):
        feed.reset(ids)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in calls]
        for (data, off, end), e, (cp, cb) in zip(calls, ev, caps):
            e[0].record()
            check(lib.vbm_ogg_feed_scan(feed._h, S, ids.ctypes.data, data.data_ptr(), off.ctypes.data, end.ctypes.data,
                                        meta.data_ptr() + 16, meta.data_ptr(), q), "vbm_ogg_feed_scan")
            if resync:
                check(lib.vbm_ogg_feed_scan_events(feed._h, meta.data_ptr() + 16 + S * FEED_INFO.itemsize, q),
                      "vbm_ogg_feed_scan_events")
            e[1].record()
            if resync:
                check(lib.vbm_ogg_feed_fill_gaps(feed._h, payload.data_ptr(), cb, offsets.data_ptr(), gp.data_ptr(),
                                                 eos.data_ptr(), gap.data_ptr(), cp, q), "vbm_ogg_feed_fill_gaps")
            else:
                check(lib.vbm_ogg_feed_fill(feed._h, payload.data_ptr(), cb, offsets.data_ptr(), gp.data_ptr(), eos.data_ptr(),
                                            cp, q), "vbm_ogg_feed_fill")
            e[2].record()
        torch.cuda.synchronize()
        st = C.c_int(-1)
        check(lib.vbm_ogg_feed_status(feed._h, C.byref(st), q), "vbm_ogg_feed_status")
        assert st.value == 0, st.value
        if rep:
            scan_ms.append(statistics.mean(e[0].elapsed_time(e[1]) for e in ev))
            fill_ms.append(statistics.mean(e[1].elapsed_time(e[2]) for e in ev))
    return statistics.median(scan_ms), statistics.median(fill_ms)


def resync_run(v, lib, check, a, runs, ids, calls, strict_feed):
    """--resync: the outputs against the strict feed's call by call, then the timed passes on the same bytes and on
    bytes with lost pages -> the JSON fields"""
    S, T = a.streams, a.writes
    kw = dict(max_page_carry=a.max_page_carry, max_packet_bytes=a.max_packet_bytes, header_cap=a.header_cap)
    feed = v.OggFeed(S, max(int(c[1][-1]) for c in calls), resync=True, **kw)
    caps = []
    strict_feed.reset(ids)
    for data, off, end in calls:
        r, w = feed.push(ids, data, end=end, offsets=off), strict_feed.push(ids, data, end=end, offsets=off)
        assert r.info.tobytes() == w.info.tobytes() and not r.left.any() and not r.gap.any().item()
        assert all(torch.equal(x, y) for x, y in ((r.payload, w.payload), (r.offsets, w.offsets),
                                                  (r.granulepos, w.granulepos), (r.eos, w.eos)))
        assert not r.events["skipped_bytes"].any() and not r.events["ignored_pages"].any() and not r.events["link"].any()
        caps.append((int(r.offsets.numel()) - 1, int(r.payload.numel())))
    scan, fill = timed_passes(lib, check, feed, ids, calls, caps, a.reps, True)
    feed.close()
    # the same streams with lost pages
    damaged, lost = lose_pages(runs * 4, a.lose)                   # four differently damaged copies of every signal
    dcalls = cut_calls(damaged, S, T)
    feed = v.OggFeed(S, max(int(c[1][-1]) for c in dcalls), resync=True, **kw)
    dcaps, gaps, left, packets = [], 0, 0, 0
    for data, off, end in dcalls:
        r = feed.push(ids, data, end=end, offsets=off)
        assert not r.info["status"].any()
        gaps, left, packets = gaps + int(r.events["gaps"].sum()), left + int(r.left.sum()), packets + int(r.counts.sum())
        dcaps.append((int(r.offsets.numel()) - 1, int(r.payload.numel())))
    dscan, dfill = timed_passes(lib, check, feed, ids, dcalls, dcaps, a.reps, True)
    feed.close()
    per_call = sum(int(c[1][-1]) for c in dcalls) / T
    return {"equal_to_strict": True, "scan_ms": scan, "fill_ms": fill,
            "lost_pages": {"rate": a.lose, "pages_lost_of_the_damaged_copies": lost, "damaged_copies": len(damaged), "gap_marks": gaps, "bytes_given_back": left,
                           "packets": packets, "ogg_bytes_per_call": per_call, "scan_ms": dscan, "fill_ms": dfill,
                           "GB_per_s": per_call / ((dscan + dfill) / 1e3) / 1e9}}


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
    ap.add_argument("--resync", action="store_true", help="measure a resync feed against the strict feed of the same run")
    ap.add_argument("--lose", type=float, default=0.01, help="--resync: the share of pages the second figure loses")
    ap.add_argument("--multiplexed", action="store_true",
                    help="measure a feed made with multiplexed=True (strict, or resync with --resync) on multiplexed mounts")
    ap.add_argument("--foreign-ratio", type=float, default=4.0, help="--multiplexed: foreign bytes per byte of the mount")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_feed.py needs a GPU: there is nothing to measure without one")

    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib, check
    from bench_demux import device_demux

    S, K, T = a.streams, a.signals, a.writes
    runs = make_streams(v, K, T, a.quality)
    ids = np.arange(S, dtype=np.int32)
    calls = cut_calls(runs, S, T)
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
    ms_scan, ms_fill = timed_passes(lib, check, feed, ids, calls, caps, a.reps, False)
    per_call = total_bytes / T
    if a.multiplexed:
        unflagged = {"scan_ms": ms_scan, "fill_ms": ms_fill}
        if a.resync:                                               # the unflagged feed of the same kind
            plain = v.OggFeed(S, max(call_bytes), max_page_carry=a.max_page_carry, max_packet_bytes=a.max_packet_bytes,
                              header_cap=a.header_cap, resync=True)
            sc, fi = timed_passes(lib, check, plain, ids, calls, caps, a.reps, True)
            plain.close()
            unflagged = {"scan_ms": sc, "fill_ms": fi}
        feed.close()
        unflagged.update(ms_per_push=unflagged["scan_ms"] + unflagged["fill_ms"], bytes_per_call=per_call)
        print(json.dumps({
            "metric": "ogg_feed_multiplexed", "mode": "resync" if a.resync else "strict", "streams": S, "signals": K,
            "quality": a.quality, "calls": T, "reps": a.reps, "packets_per_call": statistics.mean(packets_per_call),
            "same_outputs": bool(same), "unflagged_on_vorbis_only_mounts": unflagged,
            "flagged": multiplexed_run(v, lib, check, a, runs, ids, want)}), flush=True)
        return
    if a.resync:
        res = resync_run(v, lib, check, a, runs, ids, calls, feed)
        feed.close()
        res["GB_per_s"] = per_call / ((res["scan_ms"] + res["fill_ms"]) / 1e3) / 1e9
        print(json.dumps({
            "metric": "ogg_feed_resync", "streams": S, "signals": K, "quality": a.quality, "calls": T, "reps": a.reps,
            "ogg_bytes_per_call": per_call, "packets_per_call": statistics.mean(packets_per_call), "same_outputs": bool(same),
            "strict": {"scan_ms": ms_scan, "fill_ms": ms_fill, "GB_per_s": per_call / ((ms_scan + ms_fill) / 1e3) / 1e9},
            "resync": res, "scan_ratio": res["scan_ms"] / ms_scan}), flush=True)
        return
    feed.close()

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
