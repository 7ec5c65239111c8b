"""The chase phase of k_tonemask as the kernel compiles it (csrc/tone_chase.h: the closed-form step on the two masks
m and L, and chase_run), built for the host and compared with a serial restatement of seed_chase's stack walk
(tests/native/tone_chase_host.cpp): the set of surviving lines, row for row.

The step alone walks whole rows from the empty stack: every row over 2 and over 3 distinct values up to 11 lines,
every row over 4 values up to 9 lines (ties, plateaus and every order of pops a 7-line window can hold), and 20000
random rows of up to 200 lines, sorted and near-constant ones among them.

The chunked walk is the kernel's: 64-line chunks, each started from (0, 0) 16 lines ahead of its own, the check of a
chunk's start state against the left neighbour's end state, re-runs until all agree, the seven bits handed left, the
last chunk's odd lines.  The harness counts the chunks that ran again; the tests assert that rows of equal seeds do
(they cascade: a chunk's guess is wrong until its left neighbour is right) and that noise rows never do."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP = C.POINTER(C.c_int)
RUNIN = 16                      # csrc/tone_kernels.hip, launch()
SHIPPED = (585, 649, 777, 841)  # total_octave_lines of the shipped block sizes


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tone_chase") / "tone_chase_host.so")
    subprocess.check_call(["c++", "-O1", "-std=c++17", "-shared", "-fPIC",
                           "-I" + os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "tone_chase_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.tone_chase_rows.argtypes = [C.c_int, C.c_int, IP, IP, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    lib.tone_chase_rows.restype = C.c_int
    return lib


def run_rows(host, rows, lens, mode):
    """rows [nrows, pitch] int32, lens [nrows]; returns the stats (chunks, chunks that ran again, re-runs, rounds,
    L bits outside m) after asserting that every row's survivors are the serial walk's"""
    rows = np.ascontiguousarray(rows, np.int32)
    lens = np.ascontiguousarray(lens, np.int32)
    stats = (C.c_longlong * 5)()
    bad = host.tone_chase_rows(len(lens), rows.shape[1], lens.ctypes.data_as(IP), rows.ctypes.data_as(IP), mode, RUNIN, stats)
    assert bad < 0, (bad, int(lens[bad]), rows[bad, :lens[bad]].tolist()[:100])
    return list(stats)


def all_rows(values, length):
    return np.array(list(itertools.product(range(values), repeat=length)), np.int32)


@pytest.mark.parametrize("values,upto", [(2, 11), (3, 11), (4, 9)])
def test_step_every_short_row(host, values, upto):
    total = 0
    for length in range(1, upto + 1):
        rows = all_rows(values, length)
        stats = run_rows(host, rows, np.full(len(rows), length), 0)
        assert stats[4] == 0        # L stays within m
        total += len(rows)
    assert total == sum(values ** k for k in range(1, upto + 1))


def test_step_random_rows(host):
    """20000 rows of 1 .. 200 lines: uniform noise, noise over 2 .. 5 values, sorted either way, constant but for a few
    lines, random walks with ties"""
    rng = np.random.default_rng(851)
    rows = np.zeros((20000, 200), np.int32)
    lens = rng.integers(1, 201, 20000)
    for r, n in enumerate(lens):
        kind = r % 6
        if kind == 0:
            s = rng.integers(0, 1 << 20, n)
        elif kind == 1:
            s = rng.integers(0, 2 + r % 4, n)
        elif kind == 2:
            s = np.sort(rng.integers(0, 40, n))
        elif kind == 3:
            s = np.sort(rng.integers(0, 40, n))[::-1]
        elif kind == 4:
            s = np.full(n, 5)
            s[rng.integers(0, n, 1 + n // 30)] = rng.integers(3, 8, 1 + n // 30)
        else:
            s = np.cumsum(rng.integers(-1, 2, n))
        rows[r, :n] = s
    stats = run_rows(host, rows, lens, 0)
    assert stats[4] == 0


def kinds(rng, n):
    i = np.arange(n)
    return {
        "equal": np.full(n, 3),
        "period2": i % 2,
        "period3": i % 3,
        "plateau2": (i // 2) % 2,
        "plateau3": (i // 3) % 2,
        "rising": i.copy(),
        "falling": -i,
        "noise": rng.integers(0, 1 << 24, n),
        "noise3": rng.integers(0, 3, n),
    }


@pytest.mark.parametrize("n", SHIPPED)
def test_chunked_shipped_lengths(host, n):
    rng = np.random.default_rng(n)
    chunks = (n + 63) // 64
    seen = {}
    for name, s in kinds(rng, n).items():
        stats = run_rows(host, s[None, :], [n], 1)
        assert stats[0] == chunks
        seen[name] = stats[1]
    # the re-run path is taken where it must be, and only there: rows of equal seeds cascade, noise and ramps converge
    # within the run-in
    assert 2 * seen["equal"] >= chunks, seen
    assert seen["noise"] == 0 and seen["rising"] == 0 and seen["falling"] == 0, seen
    for k in range(20):
        assert run_rows(host, rng.integers(0, 1 << 24, n)[None, :], [n], 1)[1] == 0, k


def test_chunked_every_short_length(host):
    """2 .. 80 lines: one chunk, a second chunk of 1 .. 16 lines (fewer than seven: the neighbour's last lines are settled
    by the last chunk; every count of odd lines past a multiple of four)"""
    rng = np.random.default_rng(80)
    reran = 0
    for n in range(2, 81):
        for name, s in kinds(rng, n).items():
            stats = run_rows(host, s[None, :], [n], 1)
            assert stats[0] == (n + 63) // 64
            reran += stats[1]
        noise = np.stack([rng.integers(0, 4, n) for _ in range(50)])
        run_rows(host, noise, np.full(50, n), 1)
    assert reran > 0


def test_chunked_random_long_rows(host):
    """rows of every length class with few values: ties at the chunk borders, re-runs of some chunks and not others"""
    rng = np.random.default_rng(4076)
    total = [0] * 5
    for n in SHIPPED + (64, 65, 127, 128, 129, 1024):
        rows = np.stack([rng.integers(0, 2 + k % 3, n) * (rng.random(n) < (0.1, 0.5, 1.0)[k % 3]) for k in range(60)])
        total = [a + b for a, b in zip(total, run_rows(host, rows, np.full(60, n), 1))]
    assert 0 < total[1] < total[0], total
