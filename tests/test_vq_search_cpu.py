"""The residue VQ search as the kernel compiles it (csrc/vq_search.h: lattice step, exhaustive search, grouped
table reads), built for the host and compared with the oracle's orc_book_besterror over every lattice book of
shipped mode packs.  No audio input was found that reaches a lattice point without a codeword or a numerator of
2^23 and more, so those two paths are driven here: vectors on and around the book's lattice
(clamped and unclamped digits, the points whose entry is unused), values past 16 bits (the unpacked distance
loop) and past 2^23 (the integer division), with and without the packed points."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from vpk import read_vpk  # noqa: E402

PACKS = ["mode_2ch_44100_q0.5.vpk", "mode_2ch_44100_q0.1.vpk", "mode_2ch_44100_q1.vpk", "mode_1ch_44100_q0.1.vpk",
         "mode_6ch_48000_q0.3.vpk", "mode_2ch_44100_b128000.vpk", "mode_1ch_8000_q0.5.vpk"]


class OrcBook(C.Structure):          # oracle/oracle.h, orc_book
    _fields_ = [("dim", C.c_int), ("entries", C.c_int), ("maptype", C.c_int), ("q_quant", C.c_int), ("q_sequencep", C.c_int),
                ("q_min", C.c_long), ("q_delta", C.c_long), ("lengthlist", C.c_void_p), ("quantlist", C.c_void_p),
                ("nquant", C.c_int), ("codelist", C.POINTER(C.c_uint32)), ("quantvals", C.c_int), ("minval", C.c_int),
                ("delta", C.c_int)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vq") / "vq_search_host.so")
    subprocess.check_call(["c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "vq_search_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.vq_search_host.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    return lib


def used_lists(dim, entries, qv, minval, delta, ll):
    """the entries that have a codeword, ascending, with their lattice points: the odometer of lib/res0.c:362-368"""
    e = [0] * 8
    maxval = minval + delta * (qv - 1)
    uidx, upt = [], []
    for k in range(entries):
        if ll[k] > 0:
            uidx.append(k)
            upt.extend(e[:dim])
        if k + 1 >= entries:
            break
        j = 0
        while j < dim and e[j] >= maxval:
            e[j] = 0
            j += 1
        if j >= dim:
            break
        if e[j] >= 0:
            e[j] += delta
        e[j] = -e[j]
    return np.array(uidx, np.int32), np.array(upt, np.int32).reshape(-1, dim)


def vectors(rng, dim, qv, minval, delta, ll, spp):
    """partitions of spp samples: lattice points and their surroundings, clamped digits, big and huge values"""
    span = delta * (qv - 1)
    out = []
    for scale in (0.6, 1.0, 1.6, 4.0):
        out.append(rng.integers(int(minval * scale) - delta, int((minval + span) * scale) + delta + 1, (40, spp)))
    # the unused lattice points themselves, +- a little: entry digits m -> value (lib/res0.c:331-333 inverted)
    ze = qv >> 1
    hole = np.flatnonzero(ll[:qv ** dim] <= 0)
    if hole.size:
        pick = hole[rng.integers(0, hole.size, 40 * (spp // dim))]
        m = np.stack([(pick // qv ** (dim - 1 - k)) % qv for k in range(dim)], axis=1)        # digit of element k
        v = np.where(m % 2 == 1, ze - (m + 1) // 2, ze + m // 2)
        pts = (v * delta + minval).reshape(40, spp)
        out.append(pts + rng.integers(-(delta // 2), delta // 2 + 1, pts.shape))
    big = rng.integers(-100000, 100001, (12, spp))                           # past 16 bits: the unpacked distance loop
    out.append(big)
    huge = rng.integers(-40, 41, (12, spp))
    huge[:, rng.integers(0, spp, 6)] = (1 << 23) + rng.integers(-3 * max(delta, 1), 3 * max(delta, 1) + 1, 6)
    huge[6:] *= -1
    out.append(huge)
    # numerators that a float no longer holds exactly (2^24 .. 2^30): kept only where every vector of the partition
    # lands on an entry with a codeword, since the distance sums of the exhaustive search overflow an int there
    far = rng.integers(-40, 41, (400, spp)).astype(np.int64)
    at = rng.integers(0, spp, 400)
    far[np.arange(400), at] = rng.integers(1 << 24, 1 << 30, 400) * rng.choice([-1, 1], 400)
    num = far - minval + (delta >> 1 if delta != 1 else 0)
    v = np.sign(num) * (np.abs(num) // delta)                                 # C's truncating division
    m = np.clip(np.where(v < ze, ((ze - v) << 1) - 1, (v - ze) << 1), 0, qv - 1).reshape(400, spp // dim, dim)
    index = sum(m[:, :, k] * qv ** k for k in range(dim))                       # element dim-1 is the leading digit
    out.append(far[(ll[index] > 0).all(axis=1)][:24])
    return np.concatenate(out).astype(np.int32)


@pytest.mark.parametrize("pack", PACKS)
def test_partition_search_equals_the_oracle(oracle, host, pack):
    from tests import orc  # noqa: F401  (oracle fixture)
    d = read_vpk(os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "data", pack))
    oracle.lib.orc_book_lattice.argtypes = [C.c_long, C.c_long, C.c_long, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    oracle.lib.orc_book_besterror.argtypes = [C.POINTER(OrcBook), C.c_void_p]
    rng = np.random.default_rng(99)
    books = holes = searched = wide = 0
    for key in sorted(k for k in d if k.startswith("book/") and k.endswith("/head")):
        h = d[key]
        dim, entries, maptype = int(h[0]), int(h[1]), int(h[2])
        if maptype != 1 or dim > 8:
            continue
        ll = np.ascontiguousarray(d[key[:-4] + "lengthlist"], np.int8)
        lat, unpacked = (C.c_int * 3)(), (C.c_float * 2)()
        oracle.lib.orc_book_lattice(int(h[3]), int(h[4]), entries, dim, lat, unpacked)
        qv, minval, delta = lat[0], lat[1], lat[2]
        if delta < 1:
            continue
        # codewords: any injective numbering will do for the comparison (the real words are test_setup_tables' matter)
        cl = (np.arange(entries, dtype=np.uint32) * np.uint32(2654435761)) | np.uint32(1)
        uidx, upt = used_lists(dim, entries, qv, minval, delta, ll)
        pk = np.zeros((len(uidx), 8), np.int16)
        pk[:, :dim] = upt
        nrm = (upt.astype(np.int64) ** 2).sum(axis=1).astype(np.int32)
        ob = OrcBook(dim=dim, entries=entries, maptype=1, lengthlist=ll.ctypes.data, codelist=cl.ctypes.data_as(C.POINTER(C.c_uint32)),
                     quantvals=qv, minval=minval, delta=delta)
        books += 1
        holes += int((ll[:qv ** dim] <= 0).any())
        spp = 32 if 32 % dim == 0 else dim * (32 // dim)
        for packed in (True, False):
            if packed and np.abs(upt).max(initial=0) > 32767:
                continue
            for vec in vectors(rng, dim, qv, minval, delta, ll, spp):
                want_rem = vec.copy()
                want_cw, want_bits = [], 0
                for t in range(spp // dim):
                    part = want_rem[t * dim:(t + 1) * dim]
                    num = part - minval + (delta >> 1)
                    wide += int(delta != 1 and (np.abs(num) >= (1 << 23)).any())
                    e = oracle.lib.orc_book_besterror(C.byref(ob), part.ctypes.data)
                    first = 0
                    for k in range(dim - 1, -1, -1):       # the lattice entry before any search, for the count below
                        v = int(np.trunc(float(int(vec[t * dim + k]) - minval + (delta >> 1 if delta != 1 else 0)) / delta)) if abs(int(vec[t * dim + k])) < 1 << 22 else None
                        if v is None:
                            first = None
                            break
                        m = (ze_m(v, qv))
                        first = first * qv + min(max(m, 0), qv - 1)
                    searched += int(first is not None and ll[first] <= 0)
                    ln = int(ll[e]) if 0 <= e < entries else 0
                    want_cw.append((int(cl[e]) | (ln << 32)) if ln > 0 else 0)
                    want_bits += max(ln, 0)
                got_rem = vec.copy()
                got_cw = np.zeros(spp // dim, np.uint64)
                bits = host.vq_search_host(dim, entries, qv, minval, delta, ll.ctypes.data, cl.ctypes.data, len(uidx),
                                           uidx.ctypes.data, upt.ctypes.data, pk.ctypes.data if packed else None,
                                           nrm.ctypes.data if packed else None, spp, got_rem.ctypes.data, got_cw.ctypes.data)
                assert bits == want_bits and got_cw.tolist() == want_cw and np.array_equal(got_rem, want_rem), \
                    f"{pack} {key} dim {dim} qv {qv} min {minval} delta {delta} packed {packed}: vector {vec.tolist()}"
    assert books >= 8 and holes >= 1 and searched > 100 and wide > 100, (books, holes, searched, wide)


def ze_m(v, qv):
    ze = qv >> 1
    return ((ze - v) << 1) - 1 if v < ze else ((v - ze) << 1)
