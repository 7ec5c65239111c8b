"""The decoder tests' own toolkit (tests/decode_packets.py, no GPU): the forms of the one blockin model agree with each
other, and the packet-list / CSR conversions round-trip."""
import numpy as np
import pytest

from tests import vorbis_model as vm
from tests.decode_packets import as_stream, blockin, csr, join, random_stream_packets, true_granules

PAIRS = [0, 3, 14]                      # vm.PAIRS: 256/256, 256/2048, 4096/4096


@pytest.fixture(scope="module", params=PAIRS, ids=[f"{vm.PAIRS[k][0]}_{vm.PAIRS[k][1]}" for k in PAIRS])
def stream(request):
    """the 40-packet stream of the pair, failed packets inside -> (bs, status, W, page-end granule positions, eos)"""
    k = request.param
    ds, packets = random_stream_packets(k, 500 + k)
    heads = [ds.unpack(p)[:2] for p in packets]
    status = [rc for rc, _ in heads]
    W = [0 if rc else info[1] for rc, info in heads]
    g, n = true_granules(ds, packets), len(packets)
    gps = [g[j] if (status[j] == 0 and (j % 5 == 4 or j == n - 1)) else -1 for j in range(n)]
    bs = tuple(ds.blocksizes)
    ds.close()
    assert bs == vm.PAIRS[k] and sum(1 for s in status if s) >= 3 and status[-1] == 0
    return bs, status, W, gps, [0] * (n - 1) + [1]


@pytest.mark.parametrize("hs", [0, 1])
def test_all_zero_gap_marks_are_no_gap_marks(stream, hs):
    bs, status, W, gps, eos = stream
    trimmed = gps[:-1] + [gps[-1] - 301]
    for gp in (gps, trimmed, [-1] * len(gps)):
        assert blockin(bs, hs, status, W, gp, eos, [0] * len(W)) == blockin(bs, hs, status, W, gp, eos)


@pytest.mark.parametrize("hs", [0, 1])
def test_a_gap_mark_starts_the_count_over_and_keeps_the_last_block(stream, hs):
    """from a marked packet k on, the counts are those of a fresh model started at k that keeps lW"""
    bs, status, W, gps, eos = stream
    valid = [j for j in range(len(W)) if status[j] == 0]
    lowered, changed = list(gps), 0
    for k in valid[1:]:
        later = next(j for j in range(k, len(W)) if gps[j] != -1)
        lowered[later] = 5                      # a stream that lost count takes it as its position and trims to it
        gap = [int(j == k) for j in range(len(W))]
        samples, out_start, total = blockin(bs, hs, status, W, lowered, eos, gap)
        plain = blockin(bs, hs, status, W, lowered, eos)
        assert samples[:k] == plain[0][:k] and out_start[:k + 1] == plain[1][:k + 1]
        prev = max(j for j in valid if j < k)
        fresh = blockin(bs, hs, status[k:], W[k:], lowered[k:], eos[k:], lW=W[prev])
        assert samples[k:] == fresh[0] and [o - out_start[k] for o in out_start[k:]] == fresh[1], k
        assert total == out_start[k] + fresh[2]
        changed += samples != plain[0]
        lowered[later] = gps[later]
    assert changed >= len(valid) // 2                             # the marks matter: the lowered position trims
    # a mark on a failed packet waits for the next valid one
    bad = next(j for j in range(1, len(W)) if status[j])
    nxt = next(j for j in valid if j > bad)
    assert blockin(bs, hs, status, W, gps, eos, [int(j == bad) for j in range(len(W))]) == \
        blockin(bs, hs, status, W, gps, eos, [int(j == nxt) for j in range(len(W))])


def test_without_granule_positions_half_rate_is_half(stream):
    bs, status, W, _, _ = stream
    none, zero = [-1] * len(W), [0] * len(W)
    full, half = blockin(bs, 0, status, W, none, zero), blockin(bs, 1, status, W, none, zero)
    assert half[0] == [n >> 1 for n in full[0]] and half[2] == full[2] >> 1 > 0
    assert half[1] == [n >> 1 for n in full[1]]


def test_as_stream_join_and_csr_round_trip():
    rng = np.random.default_rng(7)
    rows = lambda sizes: [(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), int(rng.integers(-1, 9000)), int(k % 2))  # noqa: E731
                          for k, n in enumerate(sizes)]
    lists = [rows([5, 0, 300, 1]), [], rows([17, 2]), [(b"", -1, 1)], rows([1])]     # an empty stream between full ones
    tuples = [as_stream(r) for r in lists]
    for r, (data, offs, gp, eo) in zip(lists, tuples):
        assert (data.dtype, offs.dtype, gp.dtype, eo.dtype) == (np.uint8, np.int64, np.int64, np.uint8)
        assert len(offs) == len(r) + 1 and len(gp) == len(eo) == len(r)
        d2, o2 = csr([p[0] for p in r])
        assert np.array_equal(d2, data) and np.array_equal(o2, offs)
        assert [(data[a:b].tobytes(), int(g), int(e)) for a, b, g, e in zip(offs[:-1], offs[1:], gp, eo)] == r
    data, offs, gp, eo, first = join(tuples)
    assert first.tolist() == [0, 4, 4, 6, 7, 8] and first.dtype == np.int64 and len(offs) == 9
    for s, (d, o, g, e) in enumerate(tuples):                      # split at stream_packets: the input tuples again
        a, b = int(first[s]), int(first[s + 1])
        assert np.array_equal(data[int(offs[a]):int(offs[b])], d)
        assert np.array_equal(offs[a:b + 1] - offs[a], o)
        assert np.array_equal(gp[a:b], g) and np.array_equal(eo[a:b], e)
    one = join([as_stream([(b"", -1, 1)])])                        # a stream of one empty packet alone
    assert len(one[0]) == 0 and one[1].tolist() == [0, 0] and one[4].tolist() == [0, 1]
    none = join([])
    assert len(none[0]) == 0 and none[1].tolist() == [0] and none[4].tolist() == [0]
