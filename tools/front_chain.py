#!/usr/bin/env python3
"""The big batch's front and back chains in a kernel trace of the from-PCM bench (rocprofv3 --kernel-trace .db, e.g.
tools/gpu_pcm_trace.sh), per write, for the last N writes (default 12: the timed region of --steps 12):

  period   start to start of the full-size k_noisemask<2,4> (the big batch's front halves follow each other on one
           HIP stream: if the period is the front half's own length, the front halves are the cycle that sets the step)
  gap      from the end of the previous big k_block_state to the start of that k_noisemask, and the kernels that ran in
           it on the same HIP stream
  back     the big batch's back chain on its stream: kernels per write, and where the packet head runs relative to
           k_couple_fast

    front_chain.py results.db [N]        (or a text timeline: start_us dur_us qN sN gx,gy,gz wg name)"""
import re
import sqlite3
import sys


def load(path):
    if not path.endswith(".db"):
        rows = []
        for l in open(path):
            f = l.split()
            rows.append((float(f[0]), float(f[1]), f[2], f[3], int(f[4].split(",")[0]), int(f[4].split(",")[1]), f[6]))
        return rows
    db = sqlite3.connect(path)
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    q = (f"select d.start, d.end, d.queue_id, d.stream_id, d.grid_size_x, d.grid_size_y, s.kernel_name from {kd} d "
         f"join {ks} s on d.kernel_id=s.id order by d.start")
    rows = db.execute(q).fetchall()
    t0 = rows[0][0]
    return [((st - t0) / 1e3, (en - st) / 1e3, f"q{qu}", f"s{sm}", gx, gy, name) for st, en, qu, sm, gx, gy, name in rows]


def short(name):
    name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)
    m = re.match(r"(k_[a-z0-9_]+?)(I.*?E)?E", name)
    return name[:m.end(1)] if m else name[:24]


rows = load(sys.argv[1])
N = int(sys.argv[2]) if len(sys.argv) > 2 else 12
nm = [r for r in rows if "k_noisemaskILi2ELi4E" in r[6]]
full = max(r[4] for r in nm)
nm = [r for r in nm if r[4] == full]
qF = nm[-1][3]
front = [r for r in rows if r[3] == qF]
print(f"full-size k_noisemask<2,4>: grid {full}, {len(nm)} launches, HIP stream {qF} (hardware queue {nm[-1][2]}); the last {N}:")
print(f"{'write':>5s} {'period us':>10s} {'gap us':>8s}  kernels in the gap (us)")
periods, gaps = [], []
for k in range(len(nm) - N, len(nm)):
    cur, prev = nm[k], nm[k - 1]
    bs = [r for r in front if "k_block_state" in r[6] and r[0] < cur[0]][-1]
    inside = [r for r in front if bs[0] + bs[1] <= r[0] < cur[0]]
    periods.append(cur[0] - prev[0])
    gaps.append(cur[0] - (bs[0] + bs[1]))
    print(f"{k - len(nm) + N:5d} {periods[-1]:10.1f} {gaps[-1]:8.1f}  " + ", ".join(f"{short(r[6])} {r[1]:.0f}" for r in inside))
print(f"mean period {sum(periods) / N:.1f} us, mean gap {sum(gaps) / N:.1f} us")
# the front half's own length: first kernel after the previous block state .. this write's block state
span = []
for k in range(len(nm) - N, len(nm)):
    cur = nm[k]
    bs_next = [r for r in front if "k_block_state" in r[6] and r[0] > cur[0]]
    if bs_next:
        span.append(bs_next[0][0] + bs_next[0][1] - cur[0])
if span:
    print(f"k_noisemask start .. k_block_state end of the same batch: mean {sum(span) / len(span):.1f} us")

cf = [r for r in rows if "k_couple_fast" in r[6]]
fullc = max(r[4] for r in cf)
cf = [r for r in cf if r[4] == fullc]
qB = cf[-1][3]
back = [r for r in rows if r[3] == qB]
print(f"\nbig back chain: HIP stream {qB} (hardware queue {cf[-1][2]}); the last {N} writes:")
print(f"{'write':>5s} {'kernels':>7s} {'chain us':>9s}  head")
for k in range(len(cf) - N, len(cf)):
    c = cf[k]
    ff = [r for r in back if "k_floor_fit" in r[6] and r[0] < c[0]][-1]
    # the batch's last kernel: k_packets_out (before the packet-words change: k_copy_counted)
    last = [r for r in back if ("k_packets_out" in r[6] or "k_copy_counted" in r[6]) and r[0] > c[0]][0]
    chain = [r for r in back if ff[0] <= r[0] <= last[0]]
    h = [r for r in chain if "k_pack_head" in r[6]][0]
    where = f"k_pack_head {h[1]:.0f} us alone, starts {h[0] - (c[0] + c[1]):+.1f} us from the end of k_couple_fast ({c[1]:.0f} us)"
    print(f"{k - len(cf) + N:5d} {len(chain):7d} {last[0] + last[1] - ff[0]:9.1f}  {where}")
