"""aoTuV M7 as k_noisemask runs it with all threads (csrc/ntfix_parallel.h: per-bin and per-group bodies, a pull
instead of the source's stamps and subtractions), built for the host and compared bit for bit with a serial
restatement of the source's loops (tests/native/ntfix_host.cpp).

Rows: random ones for every row length and every shipped tonefix_end (data/common.vpk, aotuv_preset), and crafted ones
for what random rows meet rarely: plateaus and exact ties, overlapping peak ranges with different ss, peaks at the
edges of the walk, both outcomes of spectral[i] > noise[i], temp on either side of its clamp, transition peaks two to
six groups apart, thres - 2 on either side of its clamp.  The harness counts how often a row had such a case, and the
tests assert that the counts are not zero."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vpk import read_vpk  # noqa: E402

PAD = 4
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ntfix") / "ntfix_host.so")
    # -ffp-contract=off as the kernels are built: every product and sum rounds separately
    subprocess.check_call(["c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "ntfix_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.ntfix_serial.argtypes = [C.c_int, C.c_int, C.c_int, FP, FP, FP, FP]
    lib.ntfix_serial.restype = None
    lib.ntfix_parallel.argtypes = [C.c_int, C.c_int, C.c_int, FP, FP, FP, FP, C.POINTER(C.c_int)]
    lib.ntfix_parallel.restype = None
    return lib


def shipped_tonefix_ends():
    """{n: [tonefix_end of the 32, 48 and 44.1 kHz presets]} (csrc/setup_host.cpp: select = 4 * rate class + size)"""
    ints = read_vpk(os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "data", "common.vpk"))["aotuv_preset/ints"]
    return {n: [int(ints[4 * k + s, 2]) for k in range(3)] for s, n in enumerate((128, 256, 1024, 2048))}


def fp(a):
    return a.ctypes.data_as(FP)


def both(host, mode, n, nx, tone_off, noise_off, spectral, noise, counts):
    """runs the serial and the parallel form on copies of the row; returns the two noise rows as uint32"""
    row = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros(PAD, np.float32)]), np.float32)
    sp, t, o = row(spectral), row(tone_off), row(noise_off)
    a, b = row(noise), row(noise)
    host.ntfix_serial(mode, n, nx, fp(t), fp(o), fp(sp), fp(a))
    host.ntfix_parallel(mode, n, nx, fp(t), fp(o), fp(sp), fp(b), counts)
    return a.view(np.uint32), b.view(np.uint32)


def tables(rng, n, kind):
    """ntfix_noiseoffset and noiseoffset[1] rows: the clamp `test` = min(tone, noise + |noise[0]|) small, large or mixed"""
    if kind == 0:
        return rng.uniform(0, 4, n).astype(np.float32), rng.uniform(-6, 2, n).astype(np.float32)
    if kind == 1:
        return rng.uniform(20, 40, n).astype(np.float32), rng.uniform(10, 30, n).astype(np.float32)
    return rng.uniform(-2, 25, n).astype(np.float32), rng.uniform(-12, 12, n).astype(np.float32)


def random_row(rng, n, mode, k):
    """a logmdct-like row and a noise row below or above it.  Every fourth row is quantised to half dB steps: ties and
    plateaus; rows differ in how peaky they are."""
    base = np.cumsum(rng.normal(0, 1.5, n)) - rng.uniform(20, 90)
    spikes = np.where(rng.random(n) < (0.02, 0.08, 0.25)[k % 3], rng.uniform(5, 45, n), 0.0)
    sp = base + spikes + rng.normal(0, (0.5, 3.0)[(k // 3) % 2], n)
    if mode == 2:
        noise = np.repeat(rng.normal(0, 2.5, n // 8), 8) + rng.normal(0, 0.7, n) + np.cumsum(rng.normal(0, .2, n))
        noise += np.repeat(np.where(rng.random(n // 8) < 0.15, rng.uniform(2, 12, n // 8), 0.0), 8)
    else:
        noise = sp + rng.normal(-2, 6, n)
    if k % 4 == 3:
        sp, noise = np.round(sp * 2) / 2, np.round(noise * 2) / 2
    return sp.astype(np.float32), noise.astype(np.float32)


@pytest.mark.parametrize("mode,n", [(0, 128), (1, 256), (2, 1024), (2, 2048)])
def test_random_rows(host, mode, n):
    """10000 rows per row length (20000 per mode), a third of them with each shipped tonefix_end"""
    rng = np.random.default_rng(7000 + n)
    ends = shipped_tonefix_ends()[n]
    counts = (C.c_int * 3)()
    for k in range(10002):
        if k % 50 == 0:
            t, o = tables(rng, n, (k // 50) % 3)
        sp, nz = random_row(rng, n, mode, k)
        a, b = both(host, mode, n, ends[k % 3], t, o, sp, nz, counts)
        assert np.array_equal(a, b), (k, int(np.flatnonzero(a != b)[0]))
    # the rows do what they are for: many peaks, overlapping ranges; short blocks: clamped temps
    assert counts[0] > 20000 and counts[1] > 2000, list(counts)
    if mode <= 1:
        assert counts[2] > 2000, list(counts)


def run_short(host, n, nx, sp, nz, test):
    """a short-block row with the clamp `test` at every bin; returns serial row, parallel row (floats), counts"""
    t = np.full(n, test, np.float32)
    o = np.full(n, 50, np.float32)
    counts = (C.c_int * 3)()
    a, b = both(host, 0 if n == 128 else 1, n, nx, t, o, np.asarray(sp, np.float32), np.asarray(nz, np.float32), counts)
    assert np.array_equal(a, b), int(np.flatnonzero(a != b)[0])
    return a.view(np.float32)[:n], list(counts)


@pytest.mark.parametrize("n", [128, 256])
def test_short_crafted(host, n):
    nx = shipped_tonefix_ends()[n][2]
    tol = 15.0 if n == 256 else 9.0
    flat = np.full(n, -60.0)

    # plateau: bins 20 and 21 equal (neither is a strict peak), and a peak whose flanks are flat (ps and pe walk out
    # over the ties to their limits)
    sp = flat.copy(); sp[20] = sp[21] = -20.0; sp[40] = -20.0
    out, c = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    assert c[0] == 1 and np.array_equal(out[18:24], (sp - 1.0).astype(np.float32)[18:24])
    chg = out != (sp - 1.0).astype(np.float32)
    assert chg[38:44].all() and not chg[37] and not chg[44]

    # exact ties next to a peak, on a falling flank: the walk stops where the spectrum rises again
    sp = flat.copy(); sp[50] = -10.0; sp[51] = sp[52] = -30.0; sp[53] = -29.0; sp[49] = -30.0; sp[48] = -25.0
    out, c = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    assert c[0] >= 1

    # two peaks three bins apart with different heights: their [ps, pe] overlap with different ss
    sp = flat.copy(); sp[30] = -10.0; sp[33] = -25.0
    out, c = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    assert c[0] == 2 and c[1] >= 1, c
    # ... and two apart: the bin between them belongs to both
    sp = flat.copy(); sp[30] = -10.0; sp[32] = -30.0
    out, c = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    assert c[0] == 2 and c[1] >= 1, c

    # peaks at bin 4 (the first the walk tests) and at nx - 1 (the last); none at bin 3 or nx
    sp = flat.copy(); sp[4] = -10.0; sp[nx - 1] = -10.0
    out, c = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    chg = out != (sp - 1.0).astype(np.float32)
    assert c[0] == 2 and chg[4] and chg[nx - 1] and not chg[:3].any() and not chg[nx + 3:].any()
    sp = flat.copy(); sp[3] = -10.0; sp[nx] = -10.0
    out, c = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    assert c[0] == 0

    # spectral[i] > noise[i] both ways: (ss - tolerance) * .6 against the whole ss
    sp = flat.copy(); sp[60] = -10.0
    lo, _ = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    hi, _ = run_short(host, n, nx, sp, sp + 1.0, 100.0)
    assert lo[60] == np.float32(np.float32(-11.0) - np.float32(np.float32(50.0 - tol) * np.float32(.6)))
    assert hi[60] == np.float32(np.float32(-9.0) - np.float32(50.0))

    # temp above and below its clamp; a negative clamp is subtracted from every bin of [3, nx), peak or not
    out, c = run_short(host, n, nx, sp, sp - 1.0, 5.0)
    assert c[2] > 0 and out[60] == np.float32(-16.0)
    out, c = run_short(host, n, nx, sp, sp - 1.0, 1000.0)
    assert c[2] == 0
    out, c = run_short(host, n, nx, sp, sp - 1.0, -1.5)
    assert out[3] == np.float32(-59.5) and out[2] == np.float32(-61.0) and out[nx] == np.float32(-61.0)

    # below -70 dB inmod is compressed tenfold: a 60 dB peak over a -130 dB floor is 6 dB there and stays
    sp = np.full(n, -130.0); sp[60] = -75.0
    out, c = run_short(host, n, nx, sp, sp - 1.0, 100.0)
    assert c[0] == 0


def run_trans(host, n, nx, means, test, jitter=None):
    """a transition-block noise row with the given 8-bin means (plus a jitter within the groups that keeps them)"""
    nz = np.repeat(np.asarray(means, np.float64), 8)
    if jitter is not None:
        nz = nz + jitter
    nz = nz.astype(np.float32)
    t = np.full(n, test, np.float32)
    o = np.full(n, 50, np.float32)
    counts = (C.c_int * 3)()
    a, b = both(host, 2, n, nx, t, o, np.zeros(n, np.float32), nz, counts)
    assert np.array_equal(a, b), int(np.flatnonzero(a != b)[0])
    return a.view(np.float32)[:n], nz, list(counts)


@pytest.mark.parametrize("n", [1024, 2048])
def test_transition_crafted(host, n):
    nx = shipped_tonefix_ends()[n][2]
    g = n // 8
    jit = np.tile(np.array([.3, -.1, .2, -.4, .1, -.2, .3, -.2]) * 0.37, g)      # sums to 0 per group, inexact in float
    # two peaks 2 .. 6 groups apart, different thres; values that are no dyadic fractions, so that the order of the two
    # subtractions shows in the last bit
    for gap in range(2, 7):
        for first_higher in (False, True):
            m = np.full(g, 1.1)
            m[20] = 7.3 if first_higher else 4.9
            m[20 + gap] = 5.7 if first_higher else 9.1
            if gap >= 3:        # a rising flank: the second range starts three groups below its peak
                m[20 + gap - 1] = 2.3
            out, nz, c = run_trans(host, n, nx, m, 100.0, jit)
            assert c[0] == 2 and c[1] >= 1, (gap, c)
    # three peaks, 2 + 2, 3 + 3 and 2 + 4 groups apart: bins that three ranges hold
    for d1, d2 in ((2, 2), (3, 3), (2, 4), (4, 2)):
        m = np.full(g, 0.7)
        m[30], m[30 + d1], m[30 + d1 + d2] = 6.1, 8.3, 5.3
        out, nz, c = run_trans(host, n, nx, m, 100.0, jit)
        assert c[0] == 3 and c[1] >= 8, (d1, d2, c)
    # a rising flank in front of the peak: the range starts a group earlier (a = i - 3)
    m = np.full(g, 0.7); m[39], m[40] = 3.0, 9.0
    out, nz, c = run_trans(host, n, nx, m, 100.0)
    assert out[8 * 37] != nz[8 * 37] and out[8 * 37 - 1] == nz[8 * 37 - 1] and out[8 * 43] != nz[8 * 43] and out[8 * 43 + 1] == nz[8 * 43 + 1]
    m = np.full(g, 0.7); m[40] = 9.0
    out, nz, c = run_trans(host, n, nx, m, 100.0)
    assert out[8 * 38] != nz[8 * 38] and out[8 * 38 - 1] == nz[8 * 38 - 1]
    # thres - 2 on either side of the clamp, and thres on either side of 2
    m = np.full(g, 1.0); m[40] = 9.0            # thres 8: subtracts 6, or the clamp
    out, nz, c = run_trans(host, n, nx, m, 100.0)
    assert out[8 * 40] == np.float32(3.0)
    out, nz, c = run_trans(host, n, nx, m, 2.5)
    assert out[8 * 40] == np.float32(6.5)
    m[40] = 3.0                                  # thres exactly 2: no peak for the source
    out, nz, c = run_trans(host, n, nx, m, 100.0)
    assert c[0] == 0 and np.array_equal(out, nz)
    m[40] = 3.0 + 2 ** -20
    out, nz, c = run_trans(host, n, nx, m, 100.0)
    assert c[0] == 1
    # the last group the walk tests (nx / 8 - 1) is compared with the cleared 0 behind the last mean, not with group
    # nx / 8 of the row: below 0 it is no peak whatever follows, above 0 it is one; its range ends past nx
    nx8 = nx // 8
    m = np.full(g, -5.0); m[nx8 - 1] = -1.0
    out, nz, c = run_trans(host, n, nx, m, 100.0)
    assert c[0] == 0
    m = np.full(g, 5.0); m[nx8 - 1] = 9.0; m[nx8] = 20.0
    out, nz, c = run_trans(host, n, nx, m, 100.0)
    assert c[0] == 1 and out[8 * (nx8 + 2)] != nz[8 * (nx8 + 2)] and out[8 * (nx8 + 2) + 1] == nz[8 * (nx8 + 2) + 1]
