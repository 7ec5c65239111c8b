"""k_noisemask's form for rows of 128 bins and its parallel M7, and k_tonemask beside them, at the batch sizes where the
workgroups differ: the stage outputs logmdct, noise, tone, epeak and npeak and the packets of every batch, bit for
bit against the oracle.

Batch sizes, in streams (tests/stage_shapes.py: B streams side by side meet at every block type): 1, 3, 4, 5, 9, 33.
k_noisemask<8,1,2> (rows of 128 bins) gives either half of a workgroup four of its eight blocks: mono batches of 1, 3,
4, 5 and 9 short blocks are a lone block, a short first half, a full first half beside an empty second, one block in
the second half, and a tail workgroup of one; stereo batches double them (2 .. 18).  k_noisemask<2,4,1> (transition and
long blocks) sees 1, 2 and 3 blocks (mono 1 and 3, stereo 1); 33 stereo streams are 66 channel-blocks, a second tile.
2ch 44100 q-0.1 has 256 / 2048-bin rows: k_noisemask<8,1,1> and <1,16,1>.  (Every form exists with and without M7's
code: short and transition batches run the first, long batches the second.)

Signals: digital silence, then at one sample a tonal complex or loud noise switched on, and a second, louder burst
later: the short and transition blocks round both onsets hold tones (M7 peaks), the transition block follows long
blocks and is followed by one (at q-0.1 both form the mean of lb_loudnoise_fix; q0.5 never does: its normal_thresh
switches the fix off).  What the corpus holds is proved on the CPU from the oracle (test_corpus_holds_the_cases): short
blocks with overlapping peak ranges, transition blocks with peaks at most six groups apart, and at q-0.1 blocks that
form the mean."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import encode_oracle as eo
from tests import orc
from tests import stage_shapes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSAMP, FIRST, SECOND = 26624, 6000, 17000
KINDS = ("complex", "noisestep", "cluster", "sparse")
CLASSES = [(1, 44100, 0.5), (2, 44100, 0.5), (2, 44100, -0.1)]
SIZES = [1, 3, 4, 5, 9, 33]
DISTINCT = 12
STAGES = ("logmdct", "noise", "tone", "epeak", "npeak")
FP = C.POINTER(C.c_float)


def small_signal(kind, variant, ch, rate):
    """Every signal is digital silence up to sample FIRST (the same first blocks for all), begins there, and has a burst
    of 300 samples at SECOND."""
    rng = np.random.default_rng(4000 + 16 * variant + KINDS.index(kind))
    pos = np.arange(NSAMP)
    t = pos.astype(np.float64) / rate
    on = pos >= FIRST
    burst = (pos >= SECOND) & (pos < SECOND + 300)
    out = np.zeros((ch, NSAMP), np.float64)
    level = 0.7 ** variant
    for c in range(ch):
        bed = np.where(on, 1e-4 * rng.uniform(-1, 1, NSAMP), 0.0)       # digital silence before FIRST
        if kind == "complex":       # inharmonic partials of unequal level: peaks a few short-block bins apart
            f0 = 700.0 * (1 + 0.21 * variant) * (1 + 0.5 * c)
            x = sum(a * np.sin(2 * np.pi * f0 * m * t + m) for m, a in ((1, .30), (1.37, .08), (2.6, .20), (3.1, .05), (5.3, .12), (7.9, .03)))
            out[c] = bed + np.where(on, level * x, 0.0) + np.where(burst, 0.5 * np.sin(2 * np.pi * 3300.0 * t), 0.0)
        elif kind == "noisestep":   # noise from FIRST on, louder from variant to variant; tones at SECOND
            out[c] = bed + np.where(on, (0.03 * 1.5 ** variant) * rng.uniform(-1, 1, NSAMP), 0.0)
            out[c] += np.where(burst, 0.4 * np.sin(2 * np.pi * 2100.0 * t) + 0.2 * np.sin(2 * np.pi * 2900.0 * t), 0.0)
        elif kind == "cluster":     # partials 350 .. 700 Hz apart (two to four 128-bin lines), up to 9 kHz
            fs = 900.0 + np.cumsum(rng.uniform(350, 700, 14))
            x = sum(rng.uniform(.02, .12) * np.sin(2 * np.pi * f * t + k) for k, f in enumerate(fs))
            out[c] = bed + np.where(on, level * x, 0.0) + np.where(burst, 0.5 * np.sin(2 * np.pi * 4100.0 * t), 0.0)
        else:                       # two distant tones over a louder bed, a click at SECOND
            out[c] = bed * 30 + np.where(on, level * (0.3 * np.sin(2 * np.pi * 1234.0 * t) + 0.1 * np.sin(2 * np.pi * 6789.0 * (c + 1) * t)), 0.0)
            out[c, SECOND] += 0.9
    return out.astype(np.float32)


SHARED = dict(keep=("lW", "nW", "block_mode", "pcm", "packet") + STAGES, distinct=DISTINCT, make=small_signal, kinds=KINDS)


def distinct_streams(oracle, ch, rate, q):
    return eo.distinct_streams(oracle, ch, rate, q, **SHARED)


def streams_for(oracle, ch, rate, q, B, first=0):
    return eo.streams_for(oracle, ch, rate, q, B, first=first, **SHARED)


@pytest.fixture(scope="module")
def probe(oracle, tmp_path_factory):
    """tests/native/psy_probe.c against the oracle's library"""
    so = str(tmp_path_factory.mktemp("psy") / "psy_probe.so")
    build = os.path.join(ROOT, "oracle", "build")
    subprocess.check_call(["cc", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "native", "psy_probe.c"), "-o", so,
                           "-L" + build, "-loracle", "-Wl,-rpath," + build])
    lib = C.CDLL(so)
    lib.psy_probe_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.psy_probe_info.restype = None
    lib.psy_probe_m7.argtypes = [C.c_void_p, C.c_int, FP, FP, FP]
    return lib


def short_peak_ranges(sp, n, nx):
    """the peaks ntfix stamps in a short block, from its logmdct row alone (lib/psy.c:3680-3716): [(ps, pe)]"""
    tol = 15.0 if n == 256 else 9.0
    sp = sp.astype(np.float32)
    inmod = np.where(sp < -70, (-70 + (sp.astype(np.float64) + 70) * .1).astype(np.float32), sp)
    out = []
    for i in range(4, nx):
        if sp[i] > sp[i - 1] and sp[i] > sp[i + 1]:
            ps, pe = i - 1, i + 1
            for j in (i - 1, i - 2):
                if sp[j + 1] < sp[j]:
                    break
                ps = j
            for j in (i + 1, i + 2, i + 3):
                if sp[j - 1] < sp[j]:
                    break
                pe = j
            if max(np.float32(inmod[i] - inmod[ps]), np.float32(inmod[i] - inmod[pe])) > tol:
                out.append((ps, pe))
    return out


def longest_run(mask):
    best = run = 0
    for m in mask:
        run = run + 1 if m else 0
        best = max(best, run)
    return best


@pytest.mark.parametrize("ch,rate,q", CLASSES)
def test_corpus_holds_the_cases(oracle, probe, ch, rate, q):
    """(CPU) the schedule brings every block type together at every size, and the blocks hold what the GPU cases are for"""
    for B in SIZES:
        streams = streams_for(oracle, ch, rate, q, B)
        assert ss.full_batches(ss.schedule(streams), B) == {0, 1, 2, 3}, B
    for first in range(4):
        one = streams_for(oracle, ch, rate, q, 1, first)
        assert ss.full_batches(ss.schedule(one), 1) == {0, 1, 2, 3}, KINDS[first]

    setup = orc.Setup(oracle, ch, rate, q)
    info = {}
    for mode in range(4):
        v = (C.c_int * 5)()
        probe.psy_probe_info(setup.h, mode, v)
        info[mode] = list(v)
    overlap = close = need = 0
    for blocks in distinct_streams(oracle, ch, rate, q):
        last = None
        for b in blocks:
            mode = b["block_mode"]
            n, nx, n25p, n75p, has_mean = info[mode]
            for c in range(ch):
                sp = np.ascontiguousarray(b["logmdct"][c], np.float32)
                if mode <= 1 and nx:
                    r = short_peak_ranges(sp, n, nx)
                    overlap += any(r[k][1] >= r[k + 1][0] for k in range(len(r) - 1))
                elif mode == 2 and nx:
                    # a lone peak changes at most six groups and a bin (49 bins) and two ranges that do not overlap are
                    # at least seven bins apart: a longer run of changed bins is two peaks at most six groups apart
                    a, w = np.empty(n, np.float32), np.empty(n, np.float32)
                    probe.psy_probe_m7(setup.h, mode, sp.ctypes.data_as(FP), a.ctypes.data_as(FP), w.ctypes.data_as(FP))
                    close += longest_run(a.view(np.uint32) != w.view(np.uint32)) > 49
                need += bool(has_mean and last is not None and {mode, last} == {2, 3})
            last = mode
    print(f"{ch}ch {rate} q{q:g}: channel-blocks with overlapping short peak ranges {overlap}, transition blocks with peaks "
          f"<= 6 groups apart {close}, blocks that form the mean {need}")
    assert overlap >= 8 and close >= 4 and (need >= 16 or q > 0.2)


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("ch,rate,q", CLASSES)
def test_small_forms_at_batch_size(oracle, cuda, ch, rate, q, B):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(ch, rate, q)
    firsts = range(4) if B == 1 else (0,)       # a lone stream of every kind
    try:
        for first in firsts:
            streams = streams_for(oracle, ch, rate, q, B, first)
            calls = ss.schedule(streams)
            assert ss.full_batches(calls, B) == {0, 1, 2, 3}
            enc = v.Encoder(setup, B)
            try:
                ss.run_schedule(enc, cuda, streams, calls, STAGES, ch)
            finally:
                enc.close()
    finally:
        setup.close()
