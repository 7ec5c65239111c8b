"""The live range store's host twin (LiveRangeStore(..., host=True): vbm_host_live_store_*, the VBMD_HD source of
csrc/live_store.h that the kernels run too), without a device: the index goes on over appends as if the stream had come in
one piece, gap marks wait for the next valid packet, the trim rule, restarts, the argument rules, and cuts from a
snapshot."""
import numpy as np
import pytest

import vorbis_aotuv_lancer_amd as v
from tests.decode_packets import BS, EINVAL, blockin, headers_of, one_byte_corpus, one_byte_stream
from tests.live_store_cases import drop_rule, padded
from vorbis_aotuv_lancer_amd.decoder import LIVE_EBIG

RUNS = [0, 1, 63, 64, 65]          # the run lengths every splitting mixes in, beside seeded ones and "all the rest"


@pytest.fixture(scope="module")
def ds():
    d = v.DecodeSetup(headers_of(2, 44100, 0.5))
    assert d.blocksizes == BS
    yield d
    d.close()


@pytest.fixture(scope="module")
def corpus():
    return one_byte_corpus()


def splits(n, seed):
    """seeded run lengths that sum to n: empty appends, runs of 1, 63, 64, 65 and, for seed 0, everything at once"""
    if seed == 0:
        return [0, n, 0]
    rng = np.random.default_rng(seed)
    out, left = [], n
    while left:
        c = int(rng.choice(RUNS)) if rng.random() < 0.6 else int(rng.integers(0, 200))
        out.append(min(c, left))
        left -= out[-1]
    return out + [0]


def feed(store, sid, stream, runs, gap=None):
    """stream = (data, offsets, granulepos, eos) of one-byte-offset CSR form, appended run by run to slot sid"""
    data, off, gp, eos = stream
    a, res = 0, []
    for c in runs:
        o = off[a:a + c + 1] - off[a]
        res.append(store.append([sid], [c], data[off[a]:off[a + c]], o, gp[a:a + c], eos[a:a + c],
                                None if gap is None else gap[a:a + c]))
        assert res[-1].status[0] == 0
        a += c
    assert a == len(off) - 1
    return res


def whole_index(ds, stream, halfrate):
    st, sm, os_, total = v.decode_index(ds, *stream, halfrate=halfrate)
    return st, sm, os_, os_ + sm, total


def heads(stream):
    """status and W of one-byte packets, as the corpus builds them: bit 0 not audio, bit 1 the mode"""
    first = stream[0][stream[1][:-1]] if len(stream[1]) > 1 else np.zeros(0, np.uint8)
    return (first & 1).astype(int), ((first >> 1) & 1).astype(int)


# ---- 1. continuity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halfrate", [False, True])
def test_index_goes_on_over_appends(ds, corpus, halfrate):
    for si, s in enumerate(corpus):
        n = len(s[1]) - 1
        want = whole_index(ds, s, halfrate)
        scan = v.decode_index_scan_host(ds, *s, halfrate=halfrate)    # status, begin, end, out_start, totals
        assert np.array_equal(scan[3] + scan[2] - scan[1], want[3])
        snaps = []
        for seed in (0, 1 + si, 1000 + si):
            st = v.LiveRangeStore(ds, 2, max(n, 1), max(n, 1), host=True, halfrate=halfrate)
            feed(st, 1, s, splits(n, seed))
            first, status, begin, out_end, totals, data, offsets = st.snapshot()
            assert list(first) == [0, 0, n] and totals[0] == 0
            assert np.array_equal(status, want[0]), f"stream {si}: status"
            assert np.array_equal(out_end, want[3]), f"stream {si}: out_end"
            assert totals[1] == want[4] == st.totals[1], f"stream {si}: total"
            assert np.array_equal(data, s[0]) and np.array_equal(offsets, s[1]), f"stream {si}: bytes"
            assert st.stats == {"trims_by_packets": 0, "trims_by_bytes": 0}
            assert np.array_equal(begin, scan[1]), f"stream {si}: begin"
            snaps.append((status, begin, out_end, st.first_sample.copy()))
            st.close()
        # begin / end: out_end - out_start is end - begin, and begin is the same however the stream was split
        for other in snaps[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(snaps[0], other)), f"stream {si}: splitting shows"


# ---- 2. gaps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halfrate", [False, True])
def test_gap_marks_cross_appends(ds, corpus, halfrate):
    rng = np.random.default_rng(7)
    crossed = 0
    for si, s in enumerate(corpus[::3]):
        n = len(s[1]) - 1
        if n == 0:
            continue
        runs = [c for c in splits(n, 50 + si) if c]
        status, W = heads(s)
        gap = (rng.random(n) < 0.08).astype(np.uint8)
        edges = np.cumsum(runs)
        gap[edges[rng.random(len(edges)) < 0.5] - 1] = 1              # the last packet of an append
        gap[(edges[:-1])[rng.random(len(edges) - 1) < 0.5]] = 1       # the first packet of the next
        gap[np.flatnonzero(status)[::2]] = 1                          # on failed packets: the mark waits
        crossed += int(np.any(gap[edges - 1] & (status[edges - 1] != 0)))
        samples, out_start, total = blockin(BS, int(halfrate), status, W, s[2], s[3], gap=gap)
        st = v.LiveRangeStore(ds, 1, n, n, host=True, halfrate=halfrate)
        feed(st, 0, s, runs, gap=gap)
        _, got_status, _, out_end, totals, _, _ = st.snapshot()
        assert np.array_equal(got_status != 0, status != 0)
        assert np.array_equal(out_end, np.asarray(out_start, np.int64) + np.asarray(samples, np.int64)), f"stream {si}"
        assert totals[0] == total
        st.close()
    assert crossed > 0, "no pending mark crossed an append boundary"


# ---- 3. trim -----------------------------------------------------------------------------------------------------------
def check_trims(ds, stream, MP, MB, runs, halfrate):
    """append run by run; after every append the snapshot is the suffix of the untrimmed index -> the store's stats"""
    data, off, gp, eos = stream
    want = whole_index(ds, stream, halfrate)
    st = v.LiveRangeStore(ds, 1, MP, MB, host=True, halfrate=halfrate)
    a = gone = 0                      # packets appended, packets dropped
    lo_before = 0
    for c in runs:
        sizes = list(np.diff(off[gone:a + 1]))
        nb = int(off[a + c] - off[a])
        d = drop_rule(sizes, c, nb, MP, MB)
        r = st.append([0], [c], data[off[a]:off[a + c]], off[a:a + c + 1] - off[a], gp[a:a + c], eos[a:a + c])
        assert (r.status[0], r.dropped[0], r.retained[0]) == (0, d, a + c - gone - d), f"append at {a}"
        gone, a = gone + d, a + c
        first, status, begin, out_end, totals, got_data, offsets = st.snapshot()
        assert first[1] == a - gone <= MP and len(got_data) <= MB
        assert np.array_equal(status, want[0][gone:a]) and np.array_equal(out_end, want[3][gone:a]), f"index at {a}"
        assert np.array_equal(got_data, data[off[gone]:off[a]]), f"bytes at {a}"
        assert np.array_equal(offsets, off[gone:a + 1] - off[gone]), f"offsets at {a}"
        assert totals[0] == st.totals[0] == (want[3][a - 1] if a else 0)
        valid = np.flatnonzero(status == 0)
        assert st.first_sample[0] == (out_end[valid[0]] if len(valid) else totals[0]), f"first_sample at {a}"
        assert st.first_sample[0] >= lo_before
        lo_before = st.first_sample[0]
    stats = st.stats
    st.close()
    return stats


@pytest.mark.parametrize("halfrate", [False, True])
def test_trim_by_packets_and_by_bytes(ds, halfrate):
    rng = np.random.default_rng(3)
    by_p = by_b = 0
    for kind, invalid in (("jitter", 0.1), ("minus2", 0.0), ("none", 0.9)):
        s = one_byte_stream(rng, 300, invalid, kind, 1)
        runs, left = [], 300
        while left:
            runs.append(min(left, int(rng.integers(0, 9))))           # up to exactly the capacity of 8
            left -= runs[-1]
        stats = check_trims(ds, s, 8, 10 ** 6, runs + [0], halfrate)
        assert stats["trims_by_bytes"] == 0
        by_p += stats["trims_by_packets"]
        p = padded(s, rng, 40)
        runs, a = [], 0
        while a < 300:
            c = int(rng.integers(0, 13))
            while p[1][min(a + c, 300)] - p[1][a] > 200:              # a run is never above the byte capacity
                c -= 1
            runs.append(min(c, 300 - a))
            a += runs[-1]
        stats = check_trims(ds, p, 1000, 200, runs, halfrate)
        assert stats["trims_by_packets"] == 0
        by_b += stats["trims_by_bytes"]
    assert by_p > 0 and by_b > 0, "the corpus never trimmed"


def test_run_of_the_capacity_and_above(ds):
    rng = np.random.default_rng(5)
    s = one_byte_stream(rng, 40, 0.1, "jitter", 1)
    data, off, gp, eos = s
    st = v.LiveRangeStore(ds, 2, 8, 8, host=True)
    feed(st, 0, (data[:3], off[:4], gp[:3], eos[:3]), [3])
    r = st.append([0], [8], data[3:11], off[3:12] - 3, gp[3:11], eos[3:11])       # exactly both capacities
    assert (r.status[0], r.dropped[0], r.retained[0]) == (0, 3, 8)
    before = st.snapshot()
    # slot 0: capacity + 1, refused; slot 1, listed behind it in the same call, is appended
    r = st.append([0, 1], [9, 2], data[11:22], off[11:23] - 11, gp[11:22], eos[11:22])
    assert list(r.status) == [LIVE_EBIG, 0] and list(r.dropped) == [0, 0] and list(r.retained) == [8, 2]
    after = st.snapshot()
    assert after[0][1] == 8 and all(np.array_equal(x[:8], y[:8]) for x, y in zip(before[1:4], after[1:4]))
    assert np.array_equal(after[5][:8], before[5]) and np.array_equal(after[5][8:], data[20:22])
    assert st.totals[0] == before[4][0]
    st.close()


# ---- 4. restart --------------------------------------------------------------------------------------------------------
def test_restart(ds, corpus):
    s, t = corpus[200], corpus[150]
    n = len(t[1]) - 1
    st = v.LiveRangeStore(ds, 3, 5000, 5000, host=True)
    st.restart([2])                                                   # an empty slot: stays fresh
    assert st.totals[2] == st.first_sample[2] == st.packets[2] == 0
    feed(st, 0, s, [len(s[1]) - 1])
    feed(st, 1, s, [len(s[1]) - 1])
    assert st.totals[0] > 0
    with pytest.raises(v.VbmError):                                   # an id listed twice: refused, nothing restarted
        st.restart([0, 0])
    assert st.totals[0] == st.totals[1] > 0
    st.restart([0])
    assert st.totals[0] == st.first_sample[0] == st.packets[0] == st.bytes[0] == 0 and st.totals[1] > 0
    feed(st, 0, t, splits(n, 4))
    want = whole_index(ds, t, False)
    first, status, _, out_end, totals, data, _ = st.snapshot()
    assert np.array_equal(status[:n], want[0]) and np.array_equal(out_end[:n], want[3]) and totals[0] == want[4]
    assert np.array_equal(data[:len(t[0])], t[0])
    st.close()


# ---- 5. arguments ------------------------------------------------------------------------------------------------------
def test_arguments(ds):
    rng = np.random.default_rng(9)
    data, off, gp, eos = one_byte_stream(rng, 20, 0.1, "jitter", 1)
    st = v.LiveRangeStore(ds, 2, 64, 64, host=True)
    feed(st, 0, (data[:5], off[:6], gp[:5], eos[:5]), [5])
    before = st.snapshot()

    def refused(ids, counts, d, o):
        o = np.asarray(o, np.int64)
        P = len(o) - 1
        rc = v.lib.vbm_host_live_store_append(st._h, len(ids), np.asarray(ids, np.int32).ctypes.data,
                                              np.asarray(counts, np.int32).ctypes.data, d.ctypes.data, o.ctypes.data,
                                              len(d), gp[:P].ctypes.data, eos[:P].ctypes.data, None, None, None, None)
        assert rc == EINVAL
        assert all(np.array_equal(a, b) for a, b in zip(before, st.snapshot())), "a refused call changed the store"

    d4, o4 = data[5:9], off[5:10] - 5
    refused([2], [4], d4, o4)                                          # an id out of range
    refused([-1], [4], d4, o4)
    refused([1, 1], [2, 2], d4, o4)                                    # an id twice in one append
    refused([0, 1], [5, -1], d4, o4)                                   # a negative count
    refused([0, 1], [2, 2], d4, [0, 1, 3, 2, 4])                       # offsets that decrease
    refused([0, 1], [2, 2], d4, [0, 1, 2, 3, 5])                       # ... that run past the data
    refused([0, 1], [2, 2], d4, [-1, 1, 2, 3, 4])
    with pytest.raises(ValueError):
        st.append([0], [4], d4, o4[:-1])
    # a host store in the device calls
    S = np.zeros(4, np.int64)
    assert v.lib.vbm_live_store_append(st._h, 0, None, None, None, o4.ctypes.data, 0, None, None, None, None, None, None,
                                       None) == EINVAL
    assert v.lib.vbm_live_store_restart(st._h, 0, None, None, None) == EINVAL
    assert v.lib.vbm_live_store_snapshot(st._h, S.ctypes.data, None, None, None, S.ctypes.data, None, S.ctypes.data,
                                         None) == EINVAL
    cutter = v.OggCutter(1, 0, 0, host=True)
    assert v.lib.vbm_ogg_cut_ranges(cutter._h, st._h, 0, None, None, None, None, 0, None, None, None, None, 0,
                                    S.ctypes.data, S.ctypes.data, None, None, None) == EINVAL
    assert "host store" in v.lib.vbm_last_error().decode()
    cutter.close()
    # bad capacities
    for args in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, 2 ** 31)):
        with pytest.raises(v.VbmError):
            v.LiveRangeStore(ds, *args, host=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, st.snapshot()))
    st.close()


# ---- 6. cuts from a snapshot -------------------------------------------------------------------------------------------
def test_cut_from_snapshot(ds):
    """streams the cutter can page but no decoder takes (one-byte heads, seeded bytes behind them), trimmed by the byte
    cap: the twin cutter over snapshot() writes the files it writes over the same suffix of decode_index, built by hand"""
    from vorbis_aotuv_lancer_amd.stream import header_pages
    rng = np.random.default_rng(21)
    hdr = header_pages([b"\x01vorbis-id", b"\x03vorbis-comment", b"\x05vorbis-setup" * 40], 0)
    st = v.LiveRangeStore(ds, 2, 400, 6000, host=True)
    streams = [padded(one_byte_stream(rng, 260, inv, "none", 0), rng, 120) for inv in (0.0, 0.1)]
    a = [0, 0]
    gone = [0, 0]
    while min(a) < 260:
        cs = [min(int(rng.integers(0, 30)), 260 - a[i]) for i in (0, 1)]
        parts = [s[0][s[1][a[i]]:s[1][a[i] + cs[i]]] for i, s in enumerate(streams)]
        offs = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(s[1][a[i]:a[i] + cs[i] + 1])
                                                              for i, s in enumerate(streams)]))]).astype(np.int64)
        gp = np.concatenate([s[2][a[i]:a[i] + cs[i]] for i, s in enumerate(streams)])
        r = st.append([0, 1], cs, np.concatenate(parts), offs, gp, None)
        for i in (0, 1):
            gone[i] += int(r.dropped[i])
            a[i] += cs[i]
    assert st.stats["trims_by_bytes"] > 0
    snap = st.snapshot()
    # the same by hand: decode_index of each whole stream, its retained suffix
    first, status, begin, out_end, totals, data, offsets = [0], [], [], [], [], [], [np.zeros(1, np.int64)]
    for i, s in enumerate(streams):
        sts, sm, os_, total = v.decode_index(ds, s[0], s[1], s[2], None)
        g = gone[i]
        status.append(sts[g:]), out_end.append((os_ + sm)[g:]), totals.append(total)
        begin.append(np.zeros(260 - g, np.int32))                     # no granule positions: nothing is trimmed
        data.append(s[0][s[1][g]:])
        offsets.append(s[1][g + 1:] - s[1][g] + offsets[-1][-1])
        first.append(first[-1] + 260 - g)
    hand = (np.asarray(first, np.int64), np.concatenate(status), np.concatenate(begin), np.concatenate(out_end),
            np.asarray(totals, np.int64), np.concatenate(data), np.concatenate(offsets))
    assert all(np.array_equal(x, y) for x, y in zip(snap, hand))
    ids, starts, lengths = [], [], []
    for i in (0, 1):
        lo, T = int(st.first_sample[i]), int(st.totals[i])
        assert 0 < lo < T
        for s0, L in ((lo, 1), (lo, T - lo), (lo + 5, 3000), (T - 10, 50), ((lo + T) // 2, 2500)):
            ids.append(i), starts.append(s0), lengths.append(L)
    outs = []
    for index in (snap, hand):
        c = v.OggCutter(len(ids), 1 << 20, len(hdr), host=True)
        buf = np.zeros(1 << 20, np.uint8)
        off, stat, gs, gl = c.cut(index, ids, starts, lengths, [hdr] * len(ids), out=buf)
        c.close()
        assert stat[-1] == 0 and not stat[:-1].any() and (gl > 0).all()
        outs.append((buf[:off[-1]].tobytes(), list(off), list(gs), list(gl)))
    assert outs[0] == outs[1]


# ---- 7. the twin's append as a program of its own, plain and under sanitizers ----------------------------------------
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_and_run(tmp_path, flags):
    """tests/native/live_store_host.cpp: csrc/live_store.h over arrays of exactly the store's sizes, nothing of it
    loaded into Python"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "live_store_host")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-Wall", *flags,
                           "-I" + os.path.join(root, "vorbis_aotuv_lancer_amd", "csrc"), "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "native", "live_store_host.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith("live_store_host ok:"), run.stdout + run.stderr


def test_native_append_and_trim(tmp_path):
    build_and_run(tmp_path, [])


def test_native_append_and_trim_under_sanitizers(tmp_path):
    import subprocess
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    link = subprocess.run(["c++", "-std=c++17", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")],
                          capture_output=True, text=True)
    if link.returncode != 0:
        pytest.skip("the compiler does not link with " + " ".join(SANITIZE) + ": " + link.stderr.strip()[-300:])
    build_and_run(tmp_path, SANITIZE)
