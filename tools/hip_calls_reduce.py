"""rocprofv3 csv output of one run (directory) -> per host thread: its HIP calls in order and its kernel dispatches in
order; per stream: its dispatches in order.  `--digest OUT`: the short form of an OUT file that is kept in the
repository: per section the number of lines, their sha256 and the count of every name (two runs with the same calls in
the same order give the same digests; compare the OUT files themselves to see where two runs part).  (Launch -> kernel through Correlation_Id is not used for the comparison:
with several host threads launching at once the profiler's ids cross between threads.)"""
import csv, glob, re, sys
from collections import defaultdict, Counter



def digest(path):
    import hashlib
    sha = lambda lines: hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]
    sec = []
    for l in open(path):
        l = l.rstrip("\n")
        if l.startswith("----"): sec.append([l[5:], [], []]); part = 1
        elif l.strip() == "dispatches:": part = 2
        else: sec[-1][part].append(l)
    main, workers = sec[:3], sec[3:]
    names = lambda lines: "\n".join(f"  {n[:96]} x {c}" for n, c in sorted(Counter(lines).items()))
    print(f"{main[0][0]}: sha256 {sha(main[0][1])}\n{names(main[0][1])}")
    print(f"{main[1][0]}\n  " + "\n  ".join(main[1][1]))
    print(f"{len(workers)} worker threads, call lists as a sorted collection: sha256 "
          f"{sha(['|'.join(w[1]) for w in sorted(workers, key=lambda w: w[1])])}; calls per worker: "
          f"{sorted(Counter(len(w[1]) for w in workers).items())}\n{names([c for w in workers for c in w[1]])}")
    every = main[2][1] + [k for w in workers for k in w[2]]
    print(f"kernel dispatches of all threads: {len(every)}, as a sorted multiset: sha256 {sha(sorted(every))}\n{names(every)}")


if sys.argv[1] == "--digest":
    digest(sys.argv[2])
    sys.exit(0)
d, out = sys.argv[1], sys.argv[2]
api = glob.glob(d + "/**/*hip_api_trace.csv", recursive=True)
ker = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
assert api and ker, (api, ker)
NOISE = re.compile(r"^(hipGetLastError|hipPeekAtLastError|__hipPushCallConfiguration|__hipPopCallConfiguration)$")


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace(" [clone .kd]", "")
    name = re.sub(r"^(void|int) ", "", name)
    depth, o = 0, []
    for c in name:          # cut the argument list: the first '(' outside template brackets
        if c == "<": depth += 1
        elif c == ">": depth -= 1
        elif c == "(" and depth == 0: break
        o.append(c)
    return "".join(o).strip().replace(" ", "") or "<unnamed>"


disp = []
for f in ker:
    rd = csv.DictReader(open(f))
    print("kernel trace columns:", rd.fieldnames)
    for r in rd:
        disp.append((int(r["Dispatch_Id"]), r.get("Thread_Id", "?"), r.get("Stream_Id", "?"), r.get("Queue_Id", "?"),
                     r["Correlation_Id"], short(r["Kernel_Name"])))
disp.sort()
rows = []
for f in api:
    rows += list(csv.DictReader(open(f)))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
calls, order, corr_thread = defaultdict(list), [], {}
for r in rows:
    corr_thread[r["Correlation_Id"]] = r["Thread_Id"]
    if NOISE.match(r["Function"]):
        continue
    if r["Thread_Id"] not in calls:
        order.append(r["Thread_Id"])
    calls[r["Thread_Id"]].append(r["Function"])
kern = defaultdict(list)
for _, t, _, _, c, n in disp:
    kern[t if t != "?" else corr_thread.get(c, "?")].append(n)
main = max(order, key=lambda t: len(calls[t]))
body = calls[main]
cut = body.index("hipMemGetInfo") if "hipMemGetInfo" in body else len(body)
workers = sorted((calls[t], kern.get(t, [])) for t in order if t != main)
with open(out, "w") as o:
    o.write(f"---- calling thread: {cut} calls up to the teardown\n" + "\n".join(body[:cut]) + "\n")
    o.write(f"---- calling thread: teardown, {len(body) - cut} calls, counted by name\n")
    o.write("\n".join(f"{n} x {c}" for n, c in sorted(Counter(body[cut:]).items())) + "\n")
    o.write(f"---- calling thread: {len(kern.get(main, []))} kernel dispatches\n" + "\n".join(kern.get(main, [])) + "\n")
    for k, (c, kn) in enumerate(workers):
        o.write(f"---- worker {k}: {len(c)} calls, {len(kn)} dispatches\n" + "\n".join(c) + "\n  dispatches:\n" + "\n".join(kn) + "\n")
with open(out + ".teardown", "w") as o:
    o.write("\n".join(body[cut:]) + "\n")
for col, idx in (("streams", 2), ("queues", 3)):
    ids, seq = {}, defaultdict(list)
    for row in disp:
        ids.setdefault(row[idx], len(ids))
        seq[ids[row[idx]]].append(row[5])
    with open(out + "." + col, "w") as o:
        for q in sorted(seq):
            o.write(f"---- {col[:-1]} {q} ({len(seq[q])} dispatches)\n" + "\n".join(seq[q]) + "\n")
    print(col, len(seq))
print(out, "calling thread", len(body), "calls;", len(workers), "workers;", len(disp), "dispatches")
