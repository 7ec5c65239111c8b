"""The resync mode of the Ogg feed on its host twin (vbm_host_ogg_feed_create2 with VBM_OGG_FEED_RESYNC): chained live
streams, joining mid-way, lost and damaged pages.  Every comparison is exact: against the byte-serial model
(tests/ogg_resync_model.py), against the strict feed and vbm_ogg_demux on undamaged input, and against what each scenario
must leave by construction."""
import ctypes as C

import numpy as np
import pytest

from tests import ogg_feed_resync_cases as R
from tests.ogg_demux_batch import six_packet_file


def run1(blob, cuts=(), end=True, **kw):
    """one stream through the host twin, checked call by call against the model -> its call records"""
    run = R.Run("host", [blob], [cuts], end, **kw)
    R.check_against_model(run, [blob], [cuts], end)
    return run.calls[0], run.headers[0]


@pytest.mark.parametrize("step", (0,) + R.CHUNKS)
def test_undamaged_single_link_files(step):
    import vorbis_aotuv_lancer_amd as v
    for name, blob in R.good_files():
        cuts = R.cuts_every(len(blob), step) if step else []
        calls, headers = run1(blob, cuts)
        want, hdr = R.strict_packets(blob)
        assert R.joined(calls) == ({0: want} if want else {}), name
        assert headers == {0: hdr}, name
        for c in calls:
            assert (c["link"], c["left"], c["skipped"], c["ignored"], c["gaps"], c["link_bad"]) == (0, 0, 0, 0, 0, 0), name
        assert sum(c["link_started"] for c in calls) == 1
        # ... and the strict feed, call by call
        edges = [0] + cuts + [len(blob)]
        strict = v.OggFeed(1, len(blob), max_packet_bytes=R.BIG, header_cap=R.BIG, host=True)
        k = 0
        for a, b in zip(edges[:-1], edges[1:]):
            r = strict.push([0], [blob[a:b]], end=b == len(blob))
            n = int(r.counts[0])
            assert r.status == [0] and [p[0] for p in calls[k]["packets"]] == \
                [r.payload[int(r.offsets[j]):int(r.offsets[j + 1])].tobytes() for j in range(n)], (name, k)
            assert [p[1] for p in calls[k]["packets"]] == r.granulepos.tolist()
            assert [p[2] for p in calls[k]["packets"]] == r.eos.tolist()
            k += 1
        assert k == len(calls)
        strict.close()


@pytest.mark.parametrize("step", (0, 255, 4096))
def test_undamaged_chained_files(step):
    import vorbis_aotuv_lancer_amd as v
    for name, blob in R.chain_files().items():
        calls, headers = run1(blob, R.cuts_every(len(blob), step) if step else [])
        b = v.demux_ogg_device([blob], chained=True, host=True)
        nlinks = len(b.info)
        got = R.joined(calls)
        for k in range(nlinks):
            assert b.info[k]["status"] == 0, (name, k)
            p0, p1 = int(b.info[k]["packet_base"]), int(b.info[k]["packet_base"] + b.info[k]["packets"])
            want = [(b.payload[int(b.offsets[j]):int(b.offsets[j + 1])].tobytes(), int(b.granulepos[j]), int(b.eos[j]),
                     int(k > 0 and j == p0)) for j in range(p0, p1)]
            assert got.get(k, []) == want, (name, k)
            assert headers[k] == list(b.headers[k]), (name, k)
        assert sum(c["link_started"] for c in calls) == nlinks and calls[-1]["link"] == nlinks - 1
        assert all(c["skipped"] == 0 and c["ignored"] == 0 for c in calls)
        if not step:                                    # whole: every link but the last stops the call in front of the next
            assert len(calls) == nlinks and [c["left"] > 0 for c in calls] == [True] * (nlinks - 1) + [False]


def removal_sets(blob):
    ap = R.audio_pages(blob)
    return [{a} for a in ap] + [{a, b} for a, b in zip(ap[:-1], ap[1:])]


FILES = {"six": lambda: six_packet_file()[0], "paged six": R.paged_six, "long": R.long_file}


@pytest.mark.parametrize("which", sorted(FILES))
def test_page_removal(which):
    blob = FILES[which]()
    spans = [(f, l) for f, l, *_ in R.packets_by_page(blob)]
    ended_and_began = 0
    for drop in removal_sets(blob):
        calls, _ = run1(R.without_pages(blob, drop))
        want = R.survivors(blob, drop)
        assert R.joined(calls).get(0, []) == want, sorted(drop)
        assert sum(c["gaps"] for c in calls) == sum(p[3] for p in want) <= 1
        d = min(drop)
        ended_and_began += len(drop) == 1 and any(f < d == l for f, l in spans) and any(f == d < l for f, l in spans)
    if which == "long":
        assert ended_and_began >= 1                     # a removed page ended a spanning packet and began another


def test_mid_stream_join():
    for blob in (f() for f in FILES.values()):
        ap = R.audio_pages(blob)
        for j in ap[1:]:
            drop = set(range(ap[0], j))
            calls, headers = run1(R.without_pages(blob, drop))
            assert R.joined(calls).get(0, []) == R.survivors(blob, drop), j
            assert 0 in headers


@pytest.mark.parametrize("where", ("header", "lacing", "body"))
def test_damage_equals_removal(where):
    for blob in (f() for f in FILES.values()):
        R.assert_no_stray_capture(blob)
        for a in R.audio_pages(blob):
            data = R.flip(blob, a, where)
            if data is None:
                continue
            calls, _ = run1(data)
            assert R.joined(calls).get(0, []) == R.survivors(blob, {a}), (where, a)
            assert sum(c["ignored"] for c in calls) == 0


@pytest.mark.parametrize("n", (1, 3, 4, 27, 300))
def test_garbage_between_pages(n):
    blob = R.paged_six()
    ps = R.pages(blob)
    want, _ = R.strict_packets(blob)
    junk = bytes((7 * i + 1) % 251 for i in range(n))
    assert b"OggS" not in junk
    for k in range(len(ps) + 1):
        data = R.join(ps[:k]) + junk + R.join(ps[k:])
        for cuts in ([], R.cuts_every(len(data), 100)):
            calls, _ = run1(data, cuts)
            assert R.joined(calls).get(0, []) == want, (n, k)
            assert sum(c["skipped"] for c in calls) == n and sum(c["gaps"] for c in calls) == 0


def test_false_capture():
    data, want, skipped = R.false_capture_file()
    for cuts in ([], R.cuts_every(len(data), 61), R.cuts_every(len(data), 1)):
        calls, _ = run1(data, cuts)
        assert R.joined(calls) == {0: want}
        assert sum(c["skipped"] for c in calls) == skipped


@pytest.mark.parametrize("step", (0, 4096, 300, 78, 27, 1))
def test_candidate_that_claims_more_than_it_has(step):
    """the carried tail holds more whole pages than the call has records for: the walk stops there and goes on in the
    next push; no status, the same packets at every chunk size, none lost at the end"""
    data, want = R.overclaim_file()
    for end in (True, False):
        calls, _ = run1(data, R.cuts_every(len(data), step) if step else [], end)
        assert R.joined(calls) == {0: want}
        assert sum(c["gaps"] for c in calls) == 1 and sum(c["ignored"] for c in calls) == 0


def test_page_lost_while_headers_open():
    from tests import ogg_chain_cases as CH
    a, b = R.paged_six(), CH.small_links(2)[1]
    pa = R.pages(a)
    assert len(pa) == 8
    data = pa[0] + R.join(pa[2:]) + b                    # the comment / setup page of link 0 is gone
    calls, headers = run1(data)
    want, hdr = R.strict_packets(b)
    assert R.joined(calls) == {1: [want[0][:3] + (1,)] + want[1:]}
    assert headers == {1: hdr}
    # the link start; then the page that shows the loss, which makes the link bad, and its five ignored followers; then link 1
    assert [(c["link"], c["link_started"], c["link_bad"], c["headers_ready"], c["ignored"]) for c in calls] == \
        [(0, 1, 0, 0, 0), (0, 0, 1, 0, 5), (1, 1, 0, 1, 0)]


def test_foreign_pages_and_pages_after_eos_are_ignored():
    from tests import ogg_chain_cases as CH
    blob = R.paged_six()
    ps = R.pages(blob)
    foreign = [p for p in R.pages(CH.reserial(blob, 555))[1:]]          # no beginning-of-stream flag among them
    want, _ = R.strict_packets(blob)
    data = R.join(ps[:3]) + foreign[1] + R.join(ps[3:]) + foreign[2] + ps[-1]
    calls, _ = run1(data)
    assert R.joined(calls) == {0: want}
    assert sum(c["ignored"] for c in calls) == 3 and sum(c["gaps"] for c in calls) == 0
    # pages in front of any link start
    calls, _ = run1(R.join(ps[3:]))
    assert R.joined(calls) == {} and calls[0]["link"] == 0 and calls[0]["link_started"] == 0 and calls[0]["ignored"] == len(ps) - 3


def test_end_flag():
    blob = six_packet_file()[0]
    want, _ = R.strict_packets(blob)
    # a partial page at the end: dropped without a status, the slot is done
    run = R.Run("host", [blob[:-5]], [[]], True)
    R.check_against_model(run, [blob[:-5]], [[]], True)
    last = R.pages(blob)[-1]
    assert run.status == [0] and run.calls[0][-1]["skipped"] == len(last) - 5
    # end with left > 0 is not honoured in that call, but in the one that leaves nothing
    from tests import ogg_chain_cases as CH
    a, b = CH.small_links(2)
    feed = R.make_feed("host", 1, len(a) + len(b))
    r = feed.push([0], [a + b], end=True)
    assert int(r.left[0]) == len(b) and int(r.info[0]["pending"]) == 0
    r = feed.push([0], [b], end=True)
    assert int(r.left[0]) == 0 and int(r.counts[0]) == len(R.strict_packets(b)[0])
    r = feed.push([0], [a], end=False)                   # done: bytes are ignored
    assert int(r.counts[0]) == 0 and r.status == [0] and int(r.info[0]["consumed"]) == 0
    feed.reset([0])
    r = feed.push([0], [a], end=False)
    assert int(r.counts[0]) == len(R.strict_packets(a)[0]) and int(r.link[0]) == 0 and not r.gap.any()
    feed.close()


@pytest.mark.parametrize("which", ("tail", "packet", "header"))
def test_too_big_fails_its_slot_alone(which):
    blob = dict(R.good_files())["header packet spans pages" if which == "header" else "packet over three pages"]
    other = six_packet_file()[0]
    caps = {"tail": dict(max_page_carry=1000), "packet": dict(max_packet_bytes=60000), "header": dict(header_cap=65536)}[which]
    for resync in (False, True):
        feed = R.make_feed("host", 2, 2 * len(blob), resync=resync, **caps)
        status, counts = [], []
        step = 30000 if which == "tail" else len(blob)
        for a in range(0, len(blob), step):
            r = feed.push([0, 1], [blob[a:a + step], other[a:a + step]])
            status.append(list(r.status)), counts.append(r.counts.tolist())
        feed.close()
        if resync:
            assert (status, counts) == strict, which
        strict = (status, counts)
        assert status[-1][0] == R.EBIG and all(s[1] == 0 for s in status)
        assert sum(c[1] for c in counts) == 6


def test_fill_capacity_one_short_then_filled_again():
    from vorbis_aotuv_lancer_amd._lib import lib
    ps, ap = R.pages(R.paged_six()), R.audio_pages(R.paged_six())
    front, blob = R.join(ps[:ap[1]]), R.join(ps[ap[2]:])       # the second audio page is gone: the rest begins with the hole
    feed, ref = R.make_feed("host", 1, len(front) + len(blob)), R.make_feed("host", 1, len(front) + len(blob))
    assert feed.push([0], [front]).counts[0] == ref.push([0], [front]).counts[0] == 1
    want = ref.push([0], [blob])
    ref.close()
    P, B = len(want.granulepos), len(want.payload)
    from vorbis_aotuv_lancer_amd.stream import FEED_INFO
    ids, off = np.zeros(1, np.int32), np.array([0, len(blob)], np.int64)
    raw, info, totals = np.frombuffer(blob, np.uint8), np.zeros(1, FEED_INFO), np.zeros(2, np.int64)
    assert lib.vbm_host_ogg_feed_scan(feed._h, 1, ids.ctypes.data, raw.ctypes.data, off.ctypes.data, None, info.ctypes.data,
                                      totals.ctypes.data) == 0
    assert totals.tolist() == [P, B] and P == 4 and want.gap.tolist() == [1, 0, 0, 0]
    for pcap, bcap in ((P - 1, B), (P, B - 1), (P, B)):
        pay, offs = np.full(B, 0xEE, np.uint8), np.full(P + 1, -7, np.int64)
        gp, eos, gap = np.full(P, -7, np.int64), np.full(P, 0xEE, np.uint8), np.full(P, 0xEE, np.uint8)
        assert lib.vbm_host_ogg_feed_fill_gaps(feed._h, pay.ctypes.data, bcap, offs.ctypes.data, gp.ctypes.data,
                                               eos.ctypes.data, gap.ctypes.data, pcap) == 0
        st = C.c_int(-7)
        assert lib.vbm_ogg_feed_status(feed._h, C.byref(st), None) == 0
        if (pcap, bcap) != (P, B):
            assert st.value == R.ECAP and (gap == 0xEE).all() and (pay == 0xEE).all() and (offs == -7).all()
        else:
            assert st.value == 0
            for got, w in ((pay, want.payload), (offs, want.offsets), (gp, want.granulepos), (eos, want.eos), (gap, want.gap)):
                assert np.array_equal(got, w)
    feed.close()


def variants():
    blob = R.paged_six()
    ap = R.audio_pages(blob)
    from tests import ogg_chain_cases as CH
    return [R.without_pages(blob, {ap[1]}), R.flip(blob, ap[2], "body"), R.without_pages(blob, set(ap[:2])),
            R.join(R.pages(blob)[:4]) + b"\x01\x02OggX" * 3 + R.join(R.pages(blob)[4:]),
            R.without_pages(blob, {ap[0]}) + CH.small_links(2)[1], R.false_capture_file()[0], R.overclaim_file()[0]]


@pytest.mark.parametrize("kind", ("two calls", "three calls", "byte by byte"))
def test_cut_invariance(kind):
    rng = np.random.default_rng(3)
    for data in variants():
        whole = R.joined(run1(data)[0])
        if kind == "two calls":
            cut_sets = [[c] for c in range(1, len(data))]
        elif kind == "three calls":
            cut_sets = [sorted(rng.choice(np.arange(1, len(data)), 2, replace=False).tolist()) for _ in range(40)]
        else:
            cut_sets = [list(range(1, len(data)))]
        feed = R.make_feed("host", 1, len(data))
        for cuts in cut_sets:
            feed.reset([0])
            run = R.Run("host", [data], [cuts], True, feed=feed)
            R.check_against_model(run, [data], [cuts], True)
            assert R.joined(run.calls[0]) == whole
        feed.close()


def test_einval_and_strict_feeds():
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    from vorbis_aotuv_lancer_amd.stream import FEED_EVENTS, FEED_INFO
    h = C.c_void_p()
    for args in ((None, 1, 10, 100, 10, 10, 1), (C.byref(h), 0, 10, 100, 10, 10, 1), (C.byref(h), 1, -1, 100, 10, 10, 1),
                 (C.byref(h), 1, 10, 0, 10, 10, 1), (C.byref(h), 1, 10, 65308, 10, 10, 1), (C.byref(h), 1, 10, 100, 0, 10, 1),
                 (C.byref(h), 1, 10, 100, 10, 0, 1), (C.byref(h), 1, 10, 100, 10, 10, 2), (C.byref(h), 1, 10, 100, 10, 10, 3)):
        assert lib.vbm_host_ogg_feed_create2(*args) == R.EINVAL and not h
    assert b"vbm_host_ogg_feed_create2" in lib.vbm_last_error()
    ev = np.zeros(2, FEED_EVENTS)
    blob = six_packet_file()[0]
    rs = v.OggFeed(2, len(blob), host=True, resync=True)
    assert lib.vbm_host_ogg_feed_scan_events(None, ev.ctypes.data) == R.EINVAL
    assert lib.vbm_host_ogg_feed_scan_events(rs._h, ev.ctypes.data) == R.EINVAL           # no scan yet
    assert lib.vbm_ogg_feed_scan_events(rs._h, ev.ctypes.data, None) == R.EINVAL          # a host feed in a device call
    ids, off = np.zeros(1, np.int32), np.array([0, len(blob)], np.int64)
    raw, info, totals = np.frombuffer(blob, np.uint8), np.zeros(1, FEED_INFO), np.zeros(2, np.int64)
    scan = lambda f: lib.vbm_host_ogg_feed_scan(f._h, 1, ids.ctypes.data, raw.ctypes.data, off.ctypes.data, None,  # noqa: E731
                                                info.ctypes.data, totals.ctypes.data)
    assert scan(rs) == 0
    assert lib.vbm_host_ogg_feed_scan_events(rs._h, None) == R.EINVAL
    assert lib.vbm_host_ogg_feed_scan_events(rs._h, ev.ctypes.data) == 0 and ev[0]["link_started"] == 1
    P, B = int(totals[0]), int(totals[1])
    pay, offs, gp, eos, gap = np.zeros(B, np.uint8), np.zeros(P + 1, np.int64), np.zeros(P, np.int64), np.zeros(P, np.uint8), \
        np.zeros(P, np.uint8)
    fill = lambda f, *a: lib.vbm_host_ogg_feed_fill_gaps(f._h, *a)                      # noqa: E731
    good = [pay.ctypes.data, B, offs.ctypes.data, gp.ctypes.data, eos.ctypes.data, gap.ctypes.data, P]
    for k, bad in ((0, None), (1, -1), (2, None), (3, None), (4, None), (6, -1)):
        a = list(good)
        a[k] = bad
        assert fill(rs, *a) == R.EINVAL, k
        assert b"vbm_host_ogg_feed_fill_gaps" in lib.vbm_last_error()       # the entry point that was called is named
    assert lib.vbm_ogg_feed_fill_gaps(rs._h, *good, None) == R.EINVAL                    # a host feed in a device call
    a = list(good)
    a[5] = None                                                                          # no marks wanted: allowed
    assert fill(rs, *a) == 0
    rs.close()
    # a strict feed: no events; fill_gaps writes zeros
    st = v.OggFeed(2, len(blob), host=True)
    assert scan(st) == 0
    assert lib.vbm_host_ogg_feed_scan_events(st._h, ev.ctypes.data) == R.EINVAL
    gap[:] = 0xEE
    assert fill(st, *good) == 0 and not gap.any() and P == 6
    st.close()
    fresh = v.OggFeed(1, 10, host=True, resync=True)
    assert fill(fresh, *good) == R.EINVAL                                                # fill without a scan
    fresh.close()
