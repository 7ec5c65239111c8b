"""The tolerant whole-file demux on the CPU (the host twin of csrc/ogg_resync.h: vbm_host_ogg_resync_scan / _fill, through
ResyncDemuxer(host=True), demux_ogg_device(resync=True, host=True) and demux_ogg_resync) against the byte-serial model of
the resync rules (tests/ogg_resync_model.py), with the host resync feed as a second yardstick.  Everything is compared
exactly: bytes, offsets, granule positions, eos, gap marks, the headers of every entry, every event counter."""
import ctypes as C

import numpy as np
import pytest

from tests import ogg_feed_resync_cases as RC
from tests import ogg_resync_file_cases as F

IMPL = "host"


def test_the_interface_is_there():
    import vorbis_aotuv_lancer_amd as v
    links, ev = v.demux_ogg_resync(RC.paged_six())
    assert len(links) == 1 and len(links[0]) == 6 and ev.dtype.names == F.EVENTS
    b = v.demux_ogg_device([RC.paged_six()], resync=True, host=True)
    assert b.gap is not None and b.events is not None and list(b.links(0)) == [0]
    assert v.demux_ogg_device([RC.paged_six()], host=True).gap is None
    assert v.demux_ogg_device([RC.paged_six()], host=True, chained=True).events is None
    with pytest.raises(ValueError):
        v.demux_ogg_device([RC.paged_six()], resync=True, multiplexed=True, host=True)
    rd = v.ResyncDemuxer(3, 1000, host=True)
    assert rd.max_candidates == 1000 // 27 + 2 * 3 + 64
    rd.close()


def test_undamaged_files_equal_the_strict_demux():
    """entry for entry, info struct included; no mark, nothing skipped or ignored"""
    import vorbis_aotuv_lancer_amd as v
    files, chains = F.undamaged()
    for blobs in (files, chains):
        b = F.check(F.run(IMPL, blobs), blobs)
        s = v.demux_ogg_device(blobs, chained=True, host=True)
        assert s.status == [0] * len(s)
        assert b.info.tobytes() == s.info.tobytes() and b.headers == s.headers
        assert np.array_equal(b.file_links, s.file_links)
        for x, y in ((b.payload, s.payload), (b.offsets, s.offsets), (b.granulepos, s.granulepos), (b.eos, s.eos)):
            assert x.tobytes() == y.tobytes()
        assert not b.events["skipped_bytes"].any() and not b.events["ignored_pages"].any() and not b.events["links_bad"].any()
        # the only marks: the first packet of every link but a file's first
        want = np.zeros(len(b.gap), np.uint8)
        for f in range(len(blobs)):
            for e in list(b.links(f))[1:]:
                if b.packets[e]:
                    want[int(b.packet_base[e])] = 1
        assert np.array_equal(b.gap, want)
        assert b.events["gaps"].sum() == want.sum()
    assert not F.run(IMPL, files).gap.any()
    F.check_each_and_together(IMPL, files + chains)


@pytest.mark.parametrize("which", ("paged_six", "long_file"))
def test_every_audio_page_and_adjacent_pair_removed(which):
    blob = getattr(RC, which)()
    cases = F.removals(blob)
    b = F.check(F.run(IMPL, [c[0] for c in cases]), [c[0] for c in cases])
    arrays = F.batch_arrays(b)
    for f, (_, want) in enumerate(cases):
        entries, ev = F.file_result(b, f, arrays)
        assert len(entries) == 1 and entries[0][1] == want, f
        assert ev["gaps"] == sum(r[3] for r in want) and ev["links_bad"] == 0
    if which == "paged_six":
        F.check_each_and_together(IMPL, [c[0] for c in cases])


@pytest.mark.parametrize("which", ("paged_six", "long_file"))
def test_a_flipped_byte_in_header_lacing_and_body_of_every_page(which):
    blobs = F.flips(getattr(RC, which)())
    assert len(blobs) > 20
    F.check(F.run(IMPL, blobs, first=3), blobs)
    if which == "paged_six":
        F.check_each_and_together(IMPL, blobs)


def test_junk_at_every_page_boundary():
    blobs = F.junked(RC.paged_six())
    F.check_each_and_together(IMPL, blobs, firsts=(0, 1))
    b = F.run(IMPL, blobs)
    per = len(blobs) // len(F.JUNK)
    for f in range(len(blobs)):
        assert b.events[f]["skipped_bytes"] == F.JUNK[f // per] and b.events[f]["pages"] == len(RC.pages(RC.paged_six()))
    long_junk = F.junked(RC.long_file())[::7]
    F.check(F.run(IMPL, long_junk), long_junk)


def test_the_damage_of_the_feed_corpus():
    d = F.feed_damage()
    F.check_each_and_together(IMPL, list(d.values()), firsts=(0, 2))
    b = F.run(IMPL, list(d.values()))
    k = list(d).index
    blob, want, skipped = RC.false_capture_file()
    got, ev = F.file_result(b, k("false capture"))
    assert got[0][1] == want and ev["skipped_bytes"] == skipped
    got, ev = F.file_result(b, k("overclaim"))
    assert got[0][1] == RC.overclaim_file()[1] and ev["ignored_pages"] == 0 and ev["gaps"] == 1
    # the first page and the one that finds the second missing are taken; the link is bad and the rest is ignored
    rest = len(RC.pages(RC.paged_six())) - 3
    assert F.file_result(b, k("headers open, alone")) == ([], dict(zip(F.EVENTS, (1, 1, 0, 0, rest, 2))))
    assert len(list(b.links(k("headers open, then a link")))) == 1
    assert b.events[k("foreign serials")]["ignored_pages"] == 3 and b.events[k("pages after eos")]["ignored_pages"] == 3


def test_the_smallest_inputs():
    blobs = F.tiny() + F.cut_headers() + F.edge_claims()
    F.check_each_and_together(IMPL, blobs, firsts=(0, 1, 2, 3))
    for last in F.cut_headers():                         # ... each at the end of the whole buffer
        F.check(F.run(IMPL, [RC.paged_six(), last]), [RC.paged_six(), last])
    b = F.run(IMPL, F.tiny())
    assert len(b) == 0 and len(b.gap) == 0 and [len(b.links(f)) for f in range(len(F.tiny()))] == [0] * len(F.tiny())
    assert b.events["skipped_bytes"].tolist() == [len(x) for x in F.tiny()]
    e = F.edge_claims()
    b = F.run(IMPL, e)
    assert [len(b.links(f)) for f in range(len(e))] == [1, 1, 0, 1, 2, 1]
    assert b.packets.tolist()[:3] == [6, 5, 0] and b.events[2]["links_bad"] == 1 and b.events[5]["links_bad"] == 1


def test_neighbours_that_form_the_pattern_across_their_boundary():
    blobs = F.across_boundary()
    b = F.check(F.run(IMPL, blobs), blobs)
    assert b"OggS" in b"".join(blobs[0:2])[len(blobs[0]) - 3:len(blobs[0]) + 3]
    assert [len(b.links(f)) for f in range(6)] == [1, 0] * 3
    F.check_each_and_together(IMPL, blobs, firsts=(1,))


def test_a_good_page_at_every_offset():
    F.check_each_and_together(IMPL, F.shifted(), firsts=(0, 1, 2, 3))
    for k, blob in enumerate(F.shifted()):               # ... from the buffer's start
        b = F.check(F.run(IMPL, [blob, RC.paged_six()]), [blob, RC.paged_six()])
        assert b.events["skipped_bytes"].tolist() == [k, 0]


def test_search_boundaries_and_nested_pages():
    F.check_each_and_together(IMPL, F.straddles())
    n = F.nested()
    b = F.check(F.run(IMPL, n), n)
    np_ = len(RC.pages(n[0]))
    assert b.events["ignored_pages"].tolist() == [0, 1, 0, 0] and b.events["pages"].tolist() == [np_, np_ - 1, np_, np_]
    # the foreign inner page leaves a hole; the stream's own carries the lost page's number and closes it
    assert b.events["gaps"].tolist() == [0, 1, 0, 0] and b.packets.tolist() == [3, 2, 3, 3]
    F.check_each_and_together(IMPL, n)


def test_the_host_feed_agrees():
    """the second yardstick: OggFeed(host=True, resync=True) fed the whole file with end"""
    d = list(F.feed_damage().values()) + [c[0] for c in F.removals(RC.paged_six())] + F.undamaged()[1] + F.nested()
    b = F.run(IMPL, d)
    arrays = F.batch_arrays(b)
    for f, blob in enumerate(d):
        r = RC.Run("host", [blob], [[]], max_page_carry=65307)
        assert r.status == [0]
        got, ev = F.file_result(b, f, arrays)
        links = RC.joined(r.calls[0])
        want = [(r.headers[0][k], links.get(k, [])) for k in sorted(r.headers[0])]
        assert got == want, f
        assert ev["skipped_bytes"] == sum(c["skipped"] for c in r.calls[0])
        assert ev["ignored_pages"] == sum(c["ignored"] for c in r.calls[0])
        assert ev["gaps"] == sum(c["gaps"] for c in r.calls[0])
        assert ev["links_started"] == sum(c["link_started"] for c in r.calls[0])


def test_65_files():
    blobs = F.sixty_five()
    F.check(F.run(IMPL, blobs, first=1), blobs)


def test_more_candidates_and_entries_than_there_is_room_for():
    import vorbis_aotuv_lancer_amd as v
    blob, chain = F.many_candidates(), RC.chain_files()["3 links"]
    rd = F.make(IMPL, 2, len(blob) + len(chain), max_candidates=10)
    raw, off = F.pack([blob, chain])
    totals, links, events, info = rd._scan(2, raw, off, 8)
    want = (blob + chain).count(b"OggS")
    assert totals.tolist() == [0, 0, 0, 0, want, F.ECAP] and not links.any() and not info.view(np.uint8).any()
    st = C.c_int(-1)
    off1 = np.zeros(1, np.int64)
    assert v.lib.vbm_host_ogg_resync_fill(rd._h, None, 0, None, 0, off1.ctypes.data, None, None, None, 0) == 0
    assert v.lib.vbm_ogg_resync_status(rd._h, C.byref(st), None) == 0 and st.value == F.ECAP and off1[0] == 0
    b = F.check(rd.demux_joined(["f0", "f1"], raw, off, entry_cap=1), [blob, chain])      # two more tries
    assert rd.max_candidates == want and len(b) == 4
    totals, links, events, info = rd._scan(2, raw, off, 3)                            # one entry short
    assert totals[0] == 4 and totals[5] == F.ECAP and links.tolist() == [0, 1, 4] and not info.view(np.uint8).any()
    assert events.tobytes() == b.events.tobytes() and totals[1] == len(b.gap)
    rd.close()


def _fill(lib, rd, H, B, P, pad=8):
    """a host fill into buffers of these capacities with canaries behind them -> (status, [(buffer, capacity bytes)])"""
    bufs = [np.full(H + pad, 0xA5, np.uint8), np.full(B + pad, 0xA5, np.uint8), np.full((P + 1) * 8 + pad, 0xA5, np.uint8),
            np.full(P * 8 + pad, 0xA5, np.uint8), np.full(P + pad, 0xA5, np.uint8), np.full(P + pad, 0xA5, np.uint8)]
    h, p, o, g, e, ga = (x.ctypes.data for x in bufs)
    assert lib.vbm_host_ogg_resync_fill(rd._h, h, H, p, B, o, g, e, ga, P) == 0
    st = C.c_int(-1)
    assert lib.vbm_ogg_resync_status(rd._h, C.byref(st), None) == 0
    return st.value, list(zip(bufs, (H, B, (P + 1) * 8, P * 8, P, P)))


def test_each_fill_capacity_one_short():
    import vorbis_aotuv_lancer_amd as v
    blobs = list(F.feed_damage().values())
    rd = F.make(IMPL, len(blobs), sum(map(len, blobs)))
    raw, off = F.pack(blobs)
    totals, _, _, _ = rd._scan(len(blobs), raw, off, 64)
    E, P, B, H = (int(x) for x in totals[:4])
    for short in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        st, bufs = _fill(v.lib, rd, H - short[0], B - short[1], P - short[2])
        assert st == F.ECAP
        assert all((x == 0xA5).all() for x, _ in bufs), short          # nothing is written at all
    st, bufs = _fill(v.lib, rd, H, B, P)
    assert st == 0 and all((x[n:] == 0xA5).all() for x, n in bufs)
    b = F.run(IMPL, blobs)
    for (x, n), y in zip(bufs[1:], F.batch_arrays(b)):
        assert x[:n].tobytes() == y.tobytes()
    rd.close()


def test_every_einval():
    import vorbis_aotuv_lancer_amd as v
    lib, h = v.lib, C.c_void_p()
    for args in ((None, 1, 10, 10), (C.byref(h), 0, 10, 10), (C.byref(h), 1, -1, 10), (C.byref(h), 1, 10, -1)):
        assert lib.vbm_host_ogg_resync_create(*args) == F.EINVAL
        assert lib.vbm_ogg_resync_create(*args) == F.EINVAL
    blob = RC.paged_six()
    rd = F.make(IMPL, 2, len(blob))
    raw, off = F.pack([blob])
    meta = np.zeros(4096, np.uint8)
    p = meta.ctypes.data
    ok = dict(n=1, data=raw.ctypes.data, off=off.ctypes.data, ev=p + 512, links=p + 256, info=p + 1024, cap=4, tot=p)

    def scan(fn=lib.vbm_host_ogg_resync_scan, extra=(), **kw):
        a = dict(ok, **kw)
        return fn(rd._h, a["n"], a["data"], a["off"], a["ev"], a["links"], a["info"], a["cap"], a["tot"], *extra)

    seven, store = np.array([7], np.int64), np.zeros(8192, np.uint8)
    assert lib.vbm_host_ogg_resync_fill(rd._h, None, 0, None, 0, p, None, None, None, 0) == F.EINVAL       # no scan yet
    for kw in (dict(n=-1), dict(n=3), dict(off=None), dict(tot=None), dict(links=None), dict(ev=None), dict(info=None),
               dict(cap=-1), dict(data=None)):
        assert scan(**kw) == F.EINVAL, kw
    keep = [np.array(x, np.int64) for x in ((-1, 5), (5, 3), (0, len(blob) + 1))]
    for a in keep:
        assert scan(off=a.ctypes.data) == F.EINVAL, a
    assert scan(lib.vbm_ogg_resync_scan, extra=(None,)) == F.EINVAL                       # a host object in a device call
    assert lib.vbm_ogg_resync_fill(rd._h, None, 0, None, 0, p, None, None, None, 0, None) == F.EINVAL
    assert lib.vbm_ogg_resync_status(None, C.byref(C.c_int()), None) == F.EINVAL
    assert lib.vbm_ogg_resync_status(rd._h, None, None) == F.EINVAL
    assert not meta.any()
    assert scan() == 0 and scan(info=None, cap=0) == 0 and scan(n=0, ev=None, data=None, off=seven.ctypes.data) == 0
    assert scan() == 0
    fill = lambda *a: lib.vbm_host_ogg_resync_fill(rd._h, *a)
    big = store.ctypes.data
    assert fill(big, 4096, big, 4096, big, big, big, big, 64) == 0
    for a in ((big, -1, big, 0, big, big, big, big, 0), (big, 0, big, -1, big, big, big, big, 0),
              (big, 0, big, 0, big, big, big, big, -1), (big, 0, big, 0, None, big, big, big, 0),
              (None, 1, big, 0, big, big, big, big, 0), (big, 0, None, 1, big, big, big, big, 0),
              (big, 0, big, 0, big, None, big, big, 1), (big, 0, big, 0, big, big, None, big, 1),
              (big, 0, big, 0, big, big, big, None, 1)):
        assert fill(*a) == F.EINVAL, a
    rd.close()
    del keep
