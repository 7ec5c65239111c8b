#!/usr/bin/env python3
"""Per kernel: launches, FETCH_SIZE and WRITE_SIZE over the run and in the largest launch, in MiB, from a rocprofv3
--pmc FETCH_SIZE (or WRITE_SIZE; one counter per pass) --kernel-trace results .db: pmc_traffic.py results.db WRITES"""
import sqlite3, sys, re, collections
db = sqlite3.connect(sys.argv[1]); writes = int(sys.argv[2])
tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
tab = lambda p: [t for t in tabs if t.startswith(p)][0]
kd, ks, pe, pi = tab("rocpd_kernel_dispatch"), tab("rocpd_info_kernel_symbol"), tab("rocpd_pmc_event"), tab("rocpd_info_pmc")
q = (f"select s.kernel_name, i.name, sum(x.v), count(*), max(x.v) from (select e.event_id eid, e.pmc_id pid, sum(e.value) v from {pe} e group by e.event_id, e.pmc_id) x "
     f"join {kd} d on d.event_id = x.eid join {ks} s on d.kernel_id = s.id join {pi} i on i.id = x.pid group by s.kernel_name, i.name")
out = collections.defaultdict(dict); calls = {}; mx = collections.defaultdict(dict)
for name, ctr, v, c, m in db.execute(q):
    name = re.sub(r"\(.*\)", "", name); name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", name)[:44]
    out[name][ctr] = v; calls[name] = c; mx[name][ctr] = m
tf = sum(d.get("FETCH_SIZE", 0) for d in out.values()); tw = sum(d.get("WRITE_SIZE", 0) for d in out.values())
print(f"# FETCH_SIZE / WRITE_SIZE are in KiB; whole traced run ({writes} timed writes + warm-up and start-up writes)")
print(f"{'kernel':44s} {'calls':>6s} {'fetch_MiB':>10s} {'write_MiB':>10s} {'max_fetch_MiB':>13s} {'max_write_MiB':>13s}")
for k, d in sorted(out.items(), key=lambda kv: -(kv[1].get("FETCH_SIZE", 0) + kv[1].get("WRITE_SIZE", 0))):
    print(f"{k:44s} {calls[k]:6d} {d.get('FETCH_SIZE',0)/1024:10.1f} {d.get('WRITE_SIZE',0)/1024:10.1f} {mx[k].get('FETCH_SIZE',0)/1024:13.2f} {mx[k].get('WRITE_SIZE',0)/1024:13.2f}")
print(f"all kernels: fetch {tf/1024:.1f} MiB, write {tw/1024:.1f} MiB, launches {sum(calls.values())}")
