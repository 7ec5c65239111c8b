#!/usr/bin/env python3
"""The mask kernels' launches and the small jobs in a kernel trace of the from-PCM bench (rocprofv3 --kernel-trace .db,
e.g. tools/gpu_pcm_trace.sh), for the last N writes (default 12: the timed region of --steps 12):

  launches  k_noisemask / k_tonemask per instantiation, the full-size batch (the HIP stream of the full-size
            k_noisemask<2,4>) apart from the small ones (short, transition and later-round long batches)
  spans     per small job, k_prologue start .. k_block_state end on its HIP stream (the psychoacoustics behind the job's
            state waits, up to its state event), and the kernel time inside

    small_jobs.py results.db [N]        (or a text timeline: start_us dur_us qN sN gx,gy,gz wg name)"""
import gzip
import re
import sqlite3
import sys
from collections import defaultdict


def load(path):
    if not path.endswith(".db"):
        rows = []
        for l in (gzip.open(path, "rt") if path.endswith(".gz") else open(path)):
            f = l.split()
            rows.append((float(f[0]), float(f[1]), f[2], f[3], int(f[4].split(",")[0]), f[6]))
        return rows
    db = sqlite3.connect(path)
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
    ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
    q = (f"select d.start, d.end, d.queue_id, d.stream_id, d.grid_size_x, s.kernel_name from {kd} d "
         f"join {ks} s on d.kernel_id=s.id order by d.start")
    rows = db.execute(q).fetchall()
    t0 = rows[0][0]
    return [((st - t0) / 1e3, (en - st) / 1e3, f"q{qu}", f"s{sm}", gx, name) for st, en, qu, sm, gx, name in rows]


rows = load(sys.argv[1])
N = int(sys.argv[2]) if len(sys.argv) > 2 else 12

def tmpl(name):
    m = re.search(r"(k_[a-z0-9_]+)I(.*?)EEv", name)
    if not m:
        m2 = re.search(r"(k_[a-z0-9_]+)", name)
        return m2.group(1) if m2 else name[:30]
    return m.group(1) + "<" + ",".join(re.findall(r"L[ib](\d+)E", "I" + m.group(2) + "E")) + ">"


big = [r for r in rows if "k_noisemaskILi2ELi4E" in r[5]]
full = max(r[4] for r in big)
bigl = [r for r in big if r[4] == full]
t0, t1 = bigl[-N - 1][0], bigl[-1][0]      # start to start of the full-size k_noisemask: N periods
sel = [r for r in rows if t0 <= r[0] < t1]
print(f"region: the last {N} writes, {(t1 - t0) / 1e3:.2f} ms, {len(sel)} launches, kernel time summed {sum(r[1] for r in sel) / 1e3 / N:.2f} ms per write")
bigstream = bigl[-1][3]
groups = defaultdict(list)
for r in sel:
    if "k_noisemask" in r[5] or "k_tonemask" in r[5]:
        kind = "full" if r[3] == bigstream else "small"
        groups[(tmpl(r[5]), kind)].append(r[1])
print(f"{'kernel':24s} {'batch':6s} {'n':>4s} {'mean us':>8s} {'median':>8s} {'min':>7s} {'max':>7s} {'total ms':>9s}")
for (k, kind), d in sorted(groups.items()):
    d = sorted(d)
    print(f"{k:24s} {kind:6s} {len(d):4d} {sum(d) / len(d):8.1f} {d[len(d) // 2]:8.1f} {d[0]:7.1f} {d[-1]:7.1f} {sum(d) / 1e3:9.2f}")
# the small jobs: per HIP stream other than the big one, k_prologue start .. k_block_state end
spans = []
psy = []
for s in sorted({r[3] for r in sel}):
    if s == bigstream:
        continue
    cur = None
    for r in (x for x in sel if x[3] == s):
        if "k_prologue" in r[5]:
            cur = r[0]
            busy = 0.0
        if cur is not None:
            busy += r[1]
            if "k_block_state" in r[5]:
                spans.append(r[0] + r[1] - cur)
                psy.append(busy)
                cur = None
if spans:
    spans.sort()
    print(f"small jobs, k_prologue start .. k_block_state end: {len(spans)} spans, mean {sum(spans) / len(spans):.1f} us, "
          f"median {spans[len(spans) // 2]:.1f}, max {spans[-1]:.1f}; kernel time inside: mean {sum(psy) / len(psy):.1f} us")
