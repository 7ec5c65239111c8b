"""Ogg cut, host twin (vbm_host_ogg_cut_ranges, no GPU): byte for byte the rule of csrc/ogg_cut.h as ogg_cut_cases.model
restates it over OggStream; every cut demuxes to the source's headers and the packets pre .. m, indexes to the window's
length and holds whole, CRC-clean pages; refusals, capacities and argument errors."""
import numpy as np
import pytest

from tests import ogg_cut_cases as K
from tests.decode_packets import EINVAL
from tests.ogg_cut_cases import ECAP, ESHAPE


def agree(store, ranges, decodable=True):
    """twin == model over one call; -> the twin's result and the model's"""
    exp = K.expected(store, ranges)
    got = K.run_twin(store, ranges, guard=64)
    assert got[2][-1] == 0
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2][:-1], exp[2])
    assert np.array_equal(got[3], exp[3]) and np.array_equal(got[4], exp[4])
    for r in range(len(ranges)):
        assert got[0][r] == exp[0][r], f"range {r}: {ranges[r]}"
    assert (got[5][int(got[1][-1]):] == 0xa5).all()       # nothing behind the outputs
    if decodable:
        for r, (i, s, L, serial) in enumerate(ranges):
            if exp[0][r]:
                K.check_cut(store.sources[i], got[0][r], int(got[4][r]), exp[5][r], serial)
    return got, exp


@pytest.mark.parametrize("name,nrandom", [("2ch-trim", 200), ("6ch", 40), ("2ch-bad", 60), ("2ch-low", 60),
                                          ("2ch-trim-bad", 30), ("2ch-pad300", 30), ("2ch-pad2000", 30)])
def test_twin_equals_the_model(name, nrandom):
    src = K.dump_source(name)
    store = K.Store([src])
    wins = K.windows(src, nrandom)
    got, exp = agree(store, [(0, s, L, 9) for s, L in wins])
    T = src.total
    for r, (s, L) in enumerate(wins):
        if s >= T or L == 0:
            assert got[0][r] == b"" and got[2][r] == 0 and got[4][r] == 0
        elif got[2][r] == 0:
            pre, k, m = exp[5][r]
            want = (s, min(L, T - s)) if k != m else (int(src.out_start[k]), s + min(L, T - s) - int(src.out_start[k]))
            assert (int(got[3][r]), int(got[4][r])) == want
    one = [r for r in range(len(wins)) if exp[5][r] and exp[5][r][1] == exp[5][r][2] and got[2][r] == 0]
    assert len(one) >= 6 and any(got[3][r] != wins[r][0] for r in one)     # windows inside one packet, starts moved
    if "low" in name:
        assert (got[2][:-1] == ESHAPE).any() and (got[2][:-1] == 0).any()


def test_eos_trim_is_kept():
    """the cut that ends at the source's end stops where the source's lowered last granule stops"""
    src, plain = K.dump_source("2ch-trim"), K.dump_source("2ch")
    assert src.total == plain.total - 300
    got, _ = agree(K.Store([src]), [(0, src.total - 2000, 5000, 1)])
    assert got[4][0] == 2000


def test_continued_pages_with_large_packets():
    src = K.dump_source("2ch-pad20000x40")
    store = K.Store([src])
    wins = [(s, L) for s, L in K.windows(src, 10, longest=9000)]
    got, exp = agree(store, [(0, s, L, 3) for s, L in wins])
    cont = [p for out in got[0] if out for p in K.parse_pages(out) if p["flags"] & 1]
    full = [p for out in got[0] if out for p in K.parse_pages(out) if len(p["lacing"]) == 255 and p["lacing"][-1] == 255]
    assert cont and full                                  # a page reaches 255 segments inside a packet


def test_refusals_beside_accepted_ranges():
    low, big, plain = K.dump_source("2ch-low"), K.dump_source("2ch-pad40000x8"), K.dump_source("2ch")
    store = K.Store([low, big, plain])
    j = int(np.flatnonzero(low.begin != 0)[0])            # the packet whose start the source trimmed
    assert low.out_start[j] > 0
    b_win = (int(low.out_start[j - 1]) + 1, int(low.out_end[j] - low.out_start[j - 1]) + 10)     # k < j <= m
    c_win = (int(low.out_start[j]) + 1, 5)                # k == m == j
    ok_low = (int(low.out_end[j]) + 5, 3000)              # behind j: accepted
    k = 3
    a_win = (int(big.out_start[k]) + 5, 2000)             # pre and k of 40 000 bytes: 157 + 157 segments
    ranges = [(2, 1000, 3000, 1), (0,) + b_win + (2,), (0,) + ok_low + (3,), (0,) + c_win + (4,), (1,) + a_win + (5,),
              (2, 5000, 100, 6)]
    got, exp = agree(store, ranges)
    assert list(got[2][:-1]) == [0, ESHAPE, 0, ESHAPE, ESHAPE, 0]
    assert K.find(low, *b_win)[2] < j <= K.find(low, *b_win)[3] and K.find(low, *c_win)[2:] == (j, j)
    for r in (1, 3, 4):
        assert got[0][r] == b"" and got[4][r] == 0 and got[1][r] == got[1][r + 1]


def test_one_call_of_64_ranges_with_streams_repeated():
    srcs = [K.dump_source("2ch-trim"), K.dump_source("6ch"), K.dump_source("2ch-bad")]
    store = K.Store(srcs)
    rng = np.random.default_rng(8)
    ranges = []
    for r in range(64):
        i = int(rng.integers(0, 3)) if r % 5 else 0       # stream 0 again and again
        ranges.append((i, int(rng.integers(0, srcs[i].total + 100)), int(rng.integers(0, 5000)), int(rng.integers(-5, 1 << 31))))
    ranges[7] = ranges[3]                                 # the same range twice
    got, _ = agree(store, ranges)
    assert got[0][7] == got[0][3] != b""


def test_header_pages_made_under_the_cut_s_own_serial_number():
    """nothing to rewrite: the same bytes as from pages made under serial number 0, which every other test gives"""
    src = K.dump_source("2ch")
    store = K.Store([src, K.dump_source("6ch")])
    ranges = [(0, 1000, 3000, 5), (1, 2000, 3000, -7), (0, 1000, 3000, 0x7fffffff), (1, 10, 10, 5)]
    a, b = K.run_twin(store, ranges), K.run_twin(store, ranges, header_serial=None)
    assert a[0] == b[0] == K.expected(store, ranges)[0] and all(a[0])


def test_default_serial_numbers_are_the_range_indices():
    from vorbis_aotuv_lancer_amd import OggCutter, header_pages
    src = K.dump_source("2ch")
    store = K.Store([src])
    c = OggCutter(3, 1 << 16, 1 << 16, host=True)
    buf = np.zeros(1 << 16, np.uint8)
    off, stat, _, _ = c.cut(store.index(), [0, 0, 0], [100, 200, 300], [1000] * 3, [header_pages(src.headers, r) for r in range(3)],
                            out=buf)
    c.close()
    for r in range(3):
        assert buf[int(off[r]):int(off[r + 1])].tobytes() == K.model(src, 100 * (r + 1), 1000, r)[0]


def test_capacity():
    src = K.dump_source("2ch")
    store = K.Store([src])
    ranges = [(0, 1000, 4000, 1), (0, src.total + 1, 10, 2), (0, 30000, 2500, 3)]
    exp = K.expected(store, ranges)
    total = int(exp[1][-1])
    for cap in (0, total - 1):
        outs, off, stat, gs, gl, buf = K.run_twin(store, ranges, cap=cap, guard=32)
        assert stat[-1] == ECAP and outs is None and (buf == 0xa5).all()             # nothing written
        assert np.array_equal(off, exp[1]) and np.array_equal(stat[:-1], exp[2]) and np.array_equal(gl, exp[4])
    outs, off, stat, _, _, buf = K.run_twin(store, ranges, cap=total, guard=32)
    assert stat[-1] == 0 and outs == exp[0] and (buf[total:] == 0xa5).all()
    outs, off, stat, _, _, _ = K.run_twin(store, [(0, src.total, 10, 1)], cap=0)     # all empty: capacity 0 suffices
    assert stat[-1] == 0 and outs == [b""]


def test_einval():
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd import OggCutter, header_pages
    src = K.dump_source("2ch")
    store = K.Store([src])
    hp = header_pages(src.headers, 0)
    c = OggCutter(2, 1 << 16, 1 << 14, host=True)
    buf = np.zeros(1 << 16, np.uint8)

    def bad(ids, st, ln, pages=None, out=buf, index=None):
        with pytest.raises(v.VbmError, match=str(EINVAL)):
            c.cut(index or store.index(), ids, st, ln, [hp] * len(ids) if pages is None else pages, out=out)

    bad([1], [0], [10])                                   # stream ids
    bad([-1], [0], [10])
    bad([0], [-1], [10])                                  # a negative start, a negative length
    bad([0], [0], [-1])
    bad([0, 0, 0], [0, 0, 0], [1, 1, 1])                  # nranges above max_ranges
    bad([0], [0], [10], pages=[hp[:-1]])                  # header pages that are not whole pages
    bad([0], [0], [10], pages=[hp * 8])                   # ... above max_header_bytes
    # a header id out of range, which OggCutter.cut never passes: the C call itself
    first, status, begin, out_end, totals, data0, offsets = store.index()
    i32, i64 = (lambda *x: np.array(x, np.int32)), (lambda *x: np.array(x, np.int64))
    ids, st, ln, hoff, off, stat, gs, gl = i32(0), i64(0), i64(10), i64(0, len(hp)), i64(0, 0), i32(0, 0), i64(0), i64(0)
    raw = np.frombuffer(hp, np.uint8)
    for hid, want in ((0, 0), (1, EINVAL), (-1, EINVAL)):
        rc = v.lib.vbm_host_ogg_cut_ranges(c._h, 1, first.ctypes.data, status.ctypes.data, begin.ctypes.data, out_end.ctypes.data,
                                           totals.ctypes.data, data0.ctypes.data, offsets.ctypes.data, len(data0), 1,
                                           ids.ctypes.data, st.ctypes.data, ln.ctypes.data, None, 1, raw.ctypes.data,
                                           hoff.ctypes.data, i32(hid).ctypes.data, buf.ctypes.data, len(buf), off.ctypes.data,
                                           stat.ctypes.data, gs.ctypes.data, gl.ctypes.data)
        assert rc == want
    data = np.concatenate([src.data, np.zeros(4096, np.uint8)])
    ix = store.index()[:5] + (data[:len(src.data)], store.offsets)
    bad([0], [0], [10], out=data[len(src.data) - 1:], index=ix)      # the output overlaps the store by a byte
    c.cut(ix, [0], [0], [10], [hp], out=data[len(src.data):])        # behind it: fine
    big = np.zeros((1 << 16) + 1, np.uint8)
    bad([0], [0], [10], out=big)                          # out_cap above max_out_bytes
    c.close()
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        OggCutter(0, 10, 10, host=True)


SIZES = [0, 1, 254, 255, 256, 70000]


def test_paging_of_synthetic_packets():
    """undecodable packets under a made-up index: lacing of every size class, a packet of more than 255 segments"""
    rng = np.random.default_rng(4)
    sizes = [int(x) for x in rng.choice(SIZES[:5], 400)]
    for at in (50, 51, 120, 300):                         # as pre and k (refused), and behind k (continued pages)
        sizes[at] = 70000
    sizes[0] = 30
    src = K.synthetic_source(sizes)
    store = K.Store([src])
    wins = [(0, 1), (0, 4000), (100 * 48 + 5, 150), (100 * 49 + 5, 150), (100 * 50 + 5, 150), (100 * 52, 3000), (100 * 100, 100 * 60),
            (100 * 110 + 7, 100 * 250), (0, src.total), (src.total - 1, 1)]
    wins += [(int(rng.integers(0, src.total)), int(rng.integers(1, 100 * 80))) for _ in range(60)]
    got, exp = agree(store, [(0, s, L, 21) for s, L in wins], decodable=False)
    assert (got[2][:-1] == ESHAPE).any() and (got[2][:-1] == 0).sum() > 40
    lac = {v for out in got[0] if out for p in K.parse_pages(out) for v in p["lacing"]}
    assert {0, 1, 254, 255}.issubset(lac)
    assert any(p["flags"] & 1 for out in got[0] if out for p in K.parse_pages(out))


def test_many_small_packets_fill_a_page_with_segments():
    """255 packets of one segment each: pages that end at 255 segments on a packet boundary"""
    sizes = [30] + [3] * 900
    src = K.synthetic_source(sizes)
    got, _ = agree(K.Store([src]), [(0, 150, 100 * 700, 1), (0, 100 * 254 + 1, 100 * 300, 2), (0, 0, src.total, 3)], decodable=False)
    assert any(len(p["lacing"]) == 255 and not p["flags"] & 1 for p in K.parse_pages(got[0][0]))
