#!/usr/bin/env python3
"""Which branches of the oracle does a corpus of PCM take?  (CPU only, test infrastructure.)

    python tools/oracle_reach.py --corpus suite        # what the test suite feeds the encoder
    python tools/oracle_reach.py --corpus reach        # the signals of tests/reach_signals.py
    python tools/oracle_reach.py --corpus reach --markdown

The device's psy, floor and couple kernels transcribe the oracle's scalar branch trees lane by lane, and a device
test compares the two: a branch direction that no test input makes the ORACLE take is a transcribed branch nobody has
compared.  This tool copies oracle/ and include/ to a temporary directory, builds the copy with -O0 --coverage (the
committed Makefile and oracle/build/ stay as they are), pushes the corpus through tests.orc.Stream (1024 samples per
write, then end of stream) in worker processes, runs `gcov -b` and prints

  * per file, the branch directions never taken (line, branch number, source text), and
  * the execution count of every named target: a line of oracle/*.c that ends in `/* REACH: name */`.

Targets are names, not line numbers, so DESIGN.md §4 and the tests survive edits of the oracle."""
import argparse
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CFLAGS = "-O0 -g --coverage -fno-fast-math -ffp-contract=off -fPIC -std=gnu99 -I../include"
FILES = ["orc_psy.c", "orc_floor1.c", "orc_mapping.c", "orc_res0.c", "orc_envelope.c", "orc_lpc.c", "orc_book.c"]
TAG = re.compile(r"/\*\s*REACH:\s*([A-Za-z0-9_.]+)\s*\*/")


# ---- corpora: lists of dict(name, make() -> (ch, n) float32, ch, rate, q, bitrate) ---------------------------------
def _e(name, make, ch, rate, q=None, bitrate=None):
    return dict(name=name, make=make, ch=ch, rate=rate, q=q, bitrate=bitrate)


def suite_corpus():
    """The PCM of the encoder parity tests, with their seeds, levels and lengths (the file each group restates is
    named beside it).  Streams that several tests share are listed once."""
    import numpy as np
    from tests.signals import burst_signal, gen_windowed_sine, synth_signal
    from tests import vq_edge_cases as vq
    out = []

    def synth(tag, ch, rate, q, seeds, nsamp, level, bitrate=None, post=None, eos=True):
        for s in seeds:
            def make(s=s):
                x = synth_signal(ch, rate, nsamp, seed=s, level=level(s))
                return post(s, x) if post else x
            out.append(_e(f"{tag}_seed{s}", make, ch, rate, q, bitrate))
            out[-1]["eos"] = eos            # False: the test stops writing without declaring the end of the stream

    third = lambda s: 1.0 if s % 3 else 0.05
    whole = lambda secs, rate: int(secs * rate) // 1024 * 1024
    # tests/test_pipeline_gpu.py
    synth("pipeline_q5", 2, 44100, 0.5, range(100, 124), 4 * 44100, third, eos=False)
    synth("pipeline_q1", 2, 44100, 0.1, range(100, 108), 3 * 44100, third, eos=False)
    synth("pipeline_51", 6, 48000, 0.8, range(100, 106), 3 * 48000, third, eos=False)
    synth("pipeline_many", 2, 44100, 0.5, range(100, 250), int(0.7 * 44100), third, eos=False)
    # tests/test_frontend_gpu.py (level by stream index = seed - 500)
    synth("frontend", 2, 44100, 0.5, range(500, 700), whole(1.6, 44100), lambda s: third(s - 500))
    synth("frontend_policy", 2, 44100, 0.5, range(500, 540), whole(2.2, 44100), lambda s: third(s - 500))
    synth("frontend_lazy", 2, 44100, 0.5, range(640, 645), 30 * 1024, lambda s: 1.0 if (s - 640) % 2 else 0.05, eos=False)
    synth("frontend_lazy_managed", 2, 44100, None, range(640, 645), 22 * 1024, lambda s: 1.0 if (s - 640) % 2 else 0.05,
          bitrate=(144000, 128000, 112000), eos=False)
    synth("frontend_managed", 2, 44100, None, range(500, 505), whole(2.0, 44100), lambda s: third(s - 500), bitrate=128000)
    for ch, rate, q in [(2, 44100, 0.3), (2, 44100, 0.9), (2, 44100, 1.0), (2, 44100, 0.0), (2, 48000, 0.5), (2, 32000, 0.5),
                        (1, 44100, 0.5), (6, 48000, 0.3), (2, 22050, 0.5), (2, 16000, 0.5), (1, 11025, 0.5), (1, 8000, 0.5),
                        (2, 44100, -0.1), (3, 44100, 0.5), (4, 44100, 0.5), (5, 44100, 0.5), (7, 44100, 0.5), (8, 44100, 0.5),
                        (8, 48000, 0.5), (2, 96000, 0.5), (2, 44100, 0.7), (2, 48000, 0.2), (2, 48000, 0.9), (1, 44100, 0.2),
                        (1, 44100, 0.9), (2, 32000, 0.2), (2, 22050, 0.8), (6, 48000, 0.5), (6, 44100, 0.5), (6, 48000, 0.1)]:
        synth(f"frontend_class_{ch}ch_{rate}_q{q:g}", ch, rate, q, range(500, 506),
              whole(1.7 if rate >= 16000 else 4.0, rate), lambda s: third(s - 500))
    synth("frontend_ogg", 2, 44100, 0.5, [77], 50 * 1024, lambda s: 1.0)
    for n, seed in [(30, 11), (45, 12), (25, 13), (25, 14), (12, 15)]:
        synth("frontend_lockstep", 2, 44100, 0.5, [seed], n * 1024, lambda s: 1.0)
    for ch, rate, q, K in [(2, 44100, 0.5, 7), (6, 48000, 0.8, 7), (1, 8000, 0.5, 6), (2, 44100, -0.1, 5)]:
        synth(f"device_rounds_{ch}ch_{rate}_q{q:g}", ch, rate, q, range(730, 730 + K), 26 * 1024, lambda s: third(s - 730))

    def tone_with_bursts():
        nsamp = 26 * 1024
        rng = np.random.default_rng(5)
        t = np.arange(nsamp) / 44100
        x = np.stack([0.3 * np.sin(2 * np.pi * 440 * t + c) for c in range(2)]).astype(np.float32)
        for at in (6000, 13500, 20500):
            x[:, at:at + 200] += (0.6 * rng.standard_normal((2, 200))).astype(np.float32)
        return x
    out.append(_e("device_rounds_together", tone_with_bursts, 2, 44100, 0.5))

    # tests/test_managed_gpu.py
    def gap(lo, hi):
        def post(s, x):
            if s % 2:
                x[:, lo:hi] = 0
            return x
        return post
    synth("managed_blobs", 2, 44100, None, range(300, 306), int(3.5 * 44100), third, bitrate=128000, eos=False)
    synth("managed_blobs_minmax", 2, 44100, None, range(300, 306), int(3.5 * 44100), third, bitrate=(144000, 128000, 112000),
          post=lambda s, x: gap(44100, 3 * 44100)((s - 300), x), eos=False)
    synth("managed_pcm", 2, 44100, None, range(500, 505), whole(2.5, 44100), lambda s: third(s - 500), bitrate=128000)
    synth("managed_minmax_pcm", 2, 44100, None, range(700, 704), whole(4.0, 44100), lambda s: 1.0,
          bitrate=(144000, 128000, 112000), post=lambda s, x: gap(44100, 3 * 44100)((s - 700), x))
    for ch, rate, br, secs in [(1, 44100, 64000, 2.0), (6, 48000, 320000, 1.7), (2, 22050, 56000, 3.0), (2, 44100, 64000, 1.7),
                               (2, 44100, 96000, 1.7), (2, 44100, 160000, 1.7), (2, 44100, 192000, 1.7),
                               (2, 44100, 256000, 1.7), (2, 48000, 128000, 1.7)]:
        synth(f"managed_class_{ch}ch_{rate}_b{br}", ch, rate, None, range(500, 504), whole(secs, rate),
              lambda s: third(s - 500), bitrate=br)

    # tests/test_vq_edges_gpu.py
    for name, ch, rate, q, make in vq.CASES:
        out.append(_e("vq_edges_" + name, lambda make=make, ch=ch, rate=rate: make(ch, rate), ch, rate, q))

    # tests/test_api_edges_gpu.py: exact zeros, 1e-6 noise, a click in silence
    for ch, rate, q in [(2, 44100, 0.5), (6, 48000, 0.8)]:
        n = 40 * 1024

        def click(ch=ch):
            x = np.zeros((ch, n), np.float32)
            x[:, 20000:20003] = 0.9
            return x
        out.append(_e(f"api_zeros_{ch}ch", lambda ch=ch: np.zeros((ch, n), np.float32), ch, rate, q))
        out.append(_e(f"api_faint_{ch}ch", lambda ch=ch: (1e-6 * np.random.default_rng(3).standard_normal((ch, n))).astype(np.float32),
                      ch, rate, q))
        out.append(_e(f"api_click_{ch}ch", click, ch, rate, q))

    # burst_signal as tests/test_mapping_seam_gpu.py and tests/test_ordering_gpu.py draw it
    for k in range(6):
        out.append(_e(f"seam_burst_{k}", lambda k=k: burst_signal(2, 44100, 40 * 1024, seed=300 + k, period=7000), 2, 44100, 0.5))
        out.append(_e(f"ordering_burst_{k}", lambda k=k: burst_signal(2, 44100, 40 * 1024, seed=70 + k, period=5000 + 1000 * k,
                                                                     level=1.0 if k % 3 else 0.05), 2, 44100, 0.5))

    # tests/test_images_gpu.py: the correlated-channel corpus, and the synth_signal streams it puts beside the images
    from tests import image_signals as im
    for e in im.IMAGES:
        out.append(_e("images_" + e["name"], lambda e=e: e["make"](e["ch"], e["rate"]), e["ch"], e["rate"], e["q"], e["bitrate"]))
    for ch, rate, q, bitrate in im.classes():
        n = whole(im.seconds_of(ch, rate, q, bitrate), rate)
        seeds = list(range(850, 850 + max(2, 6 - len(im.images_of(ch, rate, q, bitrate)))))
        if (ch, rate, q) in [(2, 44100, 0.5), (2, 44100, -0.1), (2, 44100, 1.0), (2, 22050, 0.5), (6, 48000, 0.3)]:
            seeds += [840, 841]
        if ch == 2 and bitrate is not None:
            seeds += [860]
        tail = f"q{q:g}" if bitrate is None else "b" + "_".join(str(x) for x in (bitrate if isinstance(bitrate, tuple) else (bitrate,)))
        synth(f"images_beside_{ch}ch_{rate}_{tail}", ch, rate, q, seeds, n, lambda s: 1.0, bitrate=bitrate)

    # tests/test_reference_input_gpu.py, widened to every shipped pack: the windowed sine in one write, then the end
    for path in sorted(glob.glob(os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "data", "mode_*.vpk"))):
        m = re.match(r"mode_(\d+)ch_(\d+)_(q|b)(-?[\d.]+?)(?:_max(\d+))?(?:_min(\d+))?\.vpk", os.path.basename(path))
        ch, rate = int(m.group(1)), int(m.group(2))
        kw = dict(q=float(m.group(4))) if m.group(3) == "q" else \
            dict(bitrate=(int(m.group(5) or -1), int(m.group(4)), int(m.group(6) or -1)))
        e = _e("sine_" + os.path.basename(path)[5:-4], lambda ch=ch: np.repeat(gen_windowed_sine()[None, :], ch, axis=0), ch, rate, **kw)
        e["one_write"] = True
        out.append(e)
    return out


def reach_corpus():
    from tests.reach_signals import REACH
    return [_e(e["name"], lambda e=e: e["make"](e["ch"], e["rate"]), e["ch"], e["rate"], e["q"], e["bitrate"]) for e in REACH]


CORPORA = {"suite": suite_corpus, "reach": reach_corpus}


def entries(corpus, only=None):
    """the corpus, or those of its entries whose name contains `only`"""
    return [e for e in CORPORA[corpus]() if not only or only in e["name"]]


# ---- build, run, read -----------------------------------------------------------------------------------------------
def build_copy(work):
    shutil.copytree(os.path.join(ROOT, "oracle"), os.path.join(work, "oracle"), ignore=shutil.ignore_patterns("build", "_ref"))
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(work, "include"))
    odir = os.path.join(work, "oracle")
    subprocess.check_call(["make", "-C", odir, "-j8", "CFLAGS=" + CFLAGS], stdout=subprocess.DEVNULL)
    objs = sorted(glob.glob(os.path.join(odir, "build", "*.o")))
    so = os.path.join(odir, "build", "liboracle.so")
    subprocess.check_call(["gcc", "-shared", "--coverage", "-o", so] + objs + ["-lm"])
    return so


def run_slice(so, corpus, index, count, only=None):
    """worker process: entries index, index + count, .. of the corpus; the counters are merged into the .gcda files
    when the process ends.  Returns the number of blocks."""
    from tests import orc
    o = orc.Oracle(so)
    blocks = 0
    setups = {}
    for k, e in list(enumerate(entries(corpus, only)))[index::count]:
        key = (e["ch"], e["rate"], e["q"], e["bitrate"])
        if key not in setups:
            setups[key] = orc.Setup(o, e["ch"], e["rate"], e["q"], bitrate=e["bitrate"])
        st = orc.Stream(setups[key])
        o.lib.orc_stream_set_capture(st.v, k % 2)      # the tests run the oracle with and without stage capture
        pcm = e["make"]()
        step = pcm.shape[1] if e.get("one_write") else 1024
        for at in range(0, pcm.shape[1], step):
            st.write(pcm[:, at:at + step])
            blocks += sum(1 for _ in st.blocks())
        if e.get("eos", True):
            st.finish()
            blocks += sum(1 for _ in st.blocks())
        st.close()
    return blocks


def read_gcov(work):
    """{file: {"lines": {lineno: count}, "never": [(lineno, branch, text)], "directions": total}} from `gcov -b`"""
    odir = os.path.join(work, "oracle")
    tagged = sorted({f for f, _ in targets().values()} - set(FILES))       # read for their targets' counts only
    subprocess.check_call(["gcov", "-b", "-c", "-o", "build"] + FILES + tagged, cwd=odir, stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    res = {}
    for f in FILES + tagged:
        lines, never, total, text, cur = {}, [], 0, {}, 0
        for row in open(os.path.join(odir, f + ".gcov"), errors="replace"):
            m = re.match(r"\s*([0-9]+\*?|-|#####|=====):\s*(\d+):(.*)$", row)
            if m:
                cur = int(m.group(2))
                text[cur] = m.group(3).strip()
                if m.group(1) not in ("-",):
                    lines[cur] = 0 if m.group(1) in ("#####", "=====") else int(m.group(1).rstrip("*"))
                continue
            m = re.match(r"branch\s+(\d+)\s+(never executed|taken (\d+))", row)
            if m:
                total += 1
                if m.group(3) is None or int(m.group(3)) == 0:
                    never.append((cur, int(m.group(1)), text[cur]))
        res[f] = dict(lines=lines, never=never, directions=total)
    return res


def targets():
    """{name: (file, lineno)} of the /* REACH: name */ comments in oracle/*.c"""
    out = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "oracle", "orc_*.c"))):
        for no, row in enumerate(open(f), 1):
            for name in TAG.findall(row):
                if name in out:
                    raise SystemExit(f"REACH target {name} is defined twice")
                out[name] = (os.path.basename(f), no)
    return out


def measure(corpus, jobs=None, keep=None, only=None):
    """-> dict(blocks, files = read_gcov(), targets = {name: dict(file, line, count)})"""
    jobs = jobs or min(8, os.cpu_count() or 1)
    work = keep or tempfile.mkdtemp(prefix="oracle_reach_")
    try:
        so = build_copy(work)
        n = len(entries(corpus, only))
        if not n:
            raise SystemExit(f"no entry of corpus {corpus} has '{only}' in its name")
        jobs = max(1, min(jobs, n))
        # workers are fresh processes of this script: the coverage counters are merged into the .gcda files when a
        # process that loaded the library ends in the ordinary way
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", so, corpus, str(i), str(jobs), only or ""],
                                  stdout=subprocess.PIPE, text=True) for i in range(jobs)]
        blocks = 0
        for p in procs:
            out = p.communicate()[0]
            if p.returncode:
                raise SystemExit(f"a worker failed with status {p.returncode}")
            blocks += int(out.split()[-1])
        files = read_gcov(work)
    finally:
        if not keep:
            shutil.rmtree(work, ignore_errors=True)
    tg = {}
    for name, (f, no) in targets().items():
        tg[name] = dict(file=f, line=no, count=files.get(f, {}).get("lines", {}).get(no, 0))
    return dict(corpus=corpus, blocks=blocks, files=files, targets=tg)


def main():
    if len(sys.argv) == 7 and sys.argv[1] == "--worker":
        print(run_slice(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6] or None))
        return
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--corpus", choices=sorted(CORPORA), required=True)
    ap.add_argument("--only", metavar="TEXT", help="only the entries whose name contains TEXT (--list shows the names)")
    ap.add_argument("--list", action="store_true", help="print the corpus' entries and stop")
    ap.add_argument("--jobs", type=int, default=None, help="worker processes (default: up to 8)")
    ap.add_argument("--keep", metavar="DIR", help="build and leave the instrumented copy and the .gcov files in DIR")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the report")
    ap.add_argument("--markdown", action="store_true", help="the never-taken directions as table rows")
    a = ap.parse_args()
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)
    if a.list:
        for e in entries(a.corpus, a.only):
            print(e["name"], f"{e['ch']}ch {e['rate']}", f"q{e['q']:g}" if e["bitrate"] is None else f"bitrate {e['bitrate']}")
        return
    r = measure(a.corpus, a.jobs, a.keep, a.only)
    if a.json:
        print(json.dumps(r))
        return
    print(f"corpus {r['corpus']}: {r['blocks']} blocks")
    for f in FILES:
        d = r["files"][f]
        taken = d["directions"] - len(d["never"])
        print(f"\n{f}: {taken} of {d['directions']} branch directions taken ({100.0 * taken / max(d['directions'], 1):.1f} %)")
        for no, br, text in d["never"]:
            print(f"| `{f}:{no}` b{br} | `{text[:90]}` |" if a.markdown else f"  {f}:{no} branch {br}: {text[:110]}")
    print("\nnamed targets (executions of the tagged line):")
    for name, t in sorted(r["targets"].items(), key=lambda kv: (kv[1]["file"], kv[1]["line"])):
        print(f"  {name:32s} {t['file']}:{t['line']:<5d} {t['count']}")


if __name__ == "__main__":
    main()
