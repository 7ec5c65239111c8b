"""OggFeed(multiplexed=True) on the host twin (vbm_host_ogg_feed_* with VBM_OGG_FEED_MULTIPLEXED): the yardsticks of
tests/ogg_feed_mux_cases.py, every comparison exact."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import ogg_feed_mux_cases as X
from tests import ogg_feed_resync_cases as RS
from tests import ogg_select_cases as SEL
from tests.ogg_feed_mux_cases import EBIG, EINVAL, EOGG


def _feed(**kw):
    import vorbis_aotuv_lancer_amd as v
    kw.setdefault("max_packet_bytes", X.BIG)
    kw.setdefault("header_cap", X.BIG)
    return v.OggFeed(kw.pop("n", 1), kw.pop("call", 1 << 20), host=True, **kw)


# ---- the yardstick's own parts ---------------------------------------------------------------------------------------

def test_cut_mapping():
    """cuts at page boundaries map to page boundaries of V, the mapping is monotone, and a cut inside a kept page keeps
    its distance from the page's start"""
    for name, m in X.corpus().items():
        v = X.vorbis_only(m)
        bounds_v, at = {0}, 0
        for p, n, kept, _ in X.walk(m):
            assert X.map_cut(m, p) == at, name
            if kept:
                assert X.map_cut(m, p + n // 2) == at + n // 2, name
                assert m[p:p + n] == v[at:at + n], name
                at += n
                bounds_v.add(at)
            else:
                assert X.map_cut(m, p + n // 2) == at, name
            assert X.map_cut(m, p + n) in bounds_v, name
        assert X.map_cut(m, len(m)) == len(v) == at, name
        step = max(1, len(m) // 500)
        mapped = [X.map_cut(m, c) for c in range(0, len(m) + 1, step)]
        assert mapped == sorted(mapped) and all(b - a <= step for a, b in zip(mapped, mapped[1:])), name


def test_selection_twin_agrees_with_the_mapping():
    import vorbis_aotuv_lancer_amd as v
    for name in ("tiny", "three groups", "more than 244 segments in front of the mark"):
        m = X.corpus()[name]
        assert v.select_vorbis_stream(m) == X.vorbis_only(m), name


def test_model_without_foreign_pages_is_the_resync_model():
    """on plain streams and chains, damaged or not, MuxSlot's calls are Slot's"""
    from tests import ogg_resync_model as M
    for blob in (X.corpus()["plain stream"], X.corpus()["plain chain"], RS.without_pages(RS.paged_six(), {5})):
        cuts = X.random_cuts(blob, 3)
        assert X.model_run(blob, cuts)[1] == M.run(blob, cuts)[1]


# ---- flags -------------------------------------------------------------------------------------------------------------

def test_flags():
    from vorbis_aotuv_lancer_amd._lib import lib
    for flags, want in ((4, 0), (5, 0), (0, 0), (1, 0), (8, EINVAL), (12, EINVAL), (6, EINVAL), (7, EINVAL), (16, EINVAL)):
        h = C.c_void_p()
        assert lib.vbm_host_ogg_feed_create2(C.byref(h), 2, 1000, 100, 100, 100, flags) == want, flags
        if want == 0:
            lib.vbm_ogg_feed_destroy(h)
    import vorbis_aotuv_lancer_amd as v
    for resync in (False, True):
        f = v.OggFeed(1, 100, host=True, resync=resync, multiplexed=True)
        assert f.multiplexed and f.resync == resync
        f.close()


def test_the_default_did_not_move():
    """an unflagged feed on a multiplexed mount: strict gives VBM_EOGG at the first foreign page behind the first, resync
    starts a link at the Skeleton head page whose headers are not the audio's"""
    m = X.corpus()["skeleton first"]
    r = X.StrictRun("host", [m], [[]], multiplexed=False)
    assert r.calls[0][0]["status"] == EOGG and r.calls[0][0]["packets"] == []
    run = RS.Run("host", [m], [[]])
    first = run.calls[0][0]
    assert first["link_started"] == 1 and first["link"] == 0 and first["left"] > 0
    assert struct.unpack_from("<I", m, 14)[0] == 71                 # the Skeleton stream's serial number


# ---- yardstick 1: equivalence --------------------------------------------------------------------------------------------

def test_strict_equivalence_random_cuts():
    names = list(X.corpus())
    blobs = [X.corpus()[n] for n in names]
    cuts = [X.strict_cuts(b, X.random_cuts(b, 100 + i)) for i, b in enumerate(blobs)]
    got = X.check_strict_equivalence("host", blobs, cuts)
    for n, calls in zip(names, got.calls):
        last = calls[-1]["status"]
        chain = sum(1 for _, _, kept, head in X.walk(X.corpus()[n]) if kept and head) > 1
        assert last == (EOGG if chain or not X.vorbis_only(X.corpus()[n]) else 0) or "first page without" in n, (n, last)


def test_resync_equivalence_random_cuts():
    blobs = list(X.corpus().values())
    cuts = [X.random_cuts(b, 200 + i) for i, b in enumerate(blobs)]
    X.check_resync_equivalence("host", blobs, cuts)


@pytest.mark.parametrize("resync", [False, True])
def test_every_cut_of_a_small_mount(resync):
    """one slot per byte position, two pushes, one batch"""
    m = X.tiny()[0]
    cuts = [[c] for c in range(len(m) + 1)]
    if resync:
        X.check_resync_equivalence("host", [m] * len(cuts), cuts)
    else:
        X.check_strict_equivalence("host", [m] * len(cuts), cuts)     # a single group: no cut needs moving


@pytest.mark.parametrize("resync", [False, True])
def test_one_byte_per_call(resync):
    m = X.tiny()[0]
    cuts = [list(range(1, len(m)))]
    (X.check_resync_equivalence if resync else X.check_strict_equivalence)("host", [m], cuts)


@pytest.mark.parametrize("resync", [False, True])
@pytest.mark.parametrize("name", ["tiny", "three groups", "more than 244 segments in front of the mark"])
def test_cuts_in_foreign_pages_and_in_the_mark(resync, name):
    m = X.corpus()[name]
    cuts = [[c] for c in X.foreign_page_cuts(m) + X.mark_cuts(m)]
    cuts += [sorted(set(X.foreign_page_cuts(m))), X.mark_cuts(m)]        # ... and all of them one after the other
    if not resync:
        assert cuts == [X.strict_cuts(m, c) for c in cuts]
    (X.check_resync_equivalence if resync else X.check_strict_equivalence)("host", [m] * len(cuts), cuts)


# ---- strict mode -------------------------------------------------------------------------------------------------------

def test_strict_chain_fails_at_the_second_vorbis_head_once_it_is_whole():
    m = X.corpus()["two groups"]
    heads = [(p, n) for p, n, kept, head in X.walk(m) if kept and head]
    assert len(heads) == 2
    p, n = heads[1]
    r = X.StrictRun("host", [m], [[p, p + 27, p + n - 1, p + n]], end=False)
    assert [c["status"] for c in r.calls[0]] == [0, 0, 0, EOGG, EOGG]
    first = X.vorbis_only(m)[:X.map_cut(m, p)]
    want = X.StrictRun("host", [first], [[]], multiplexed=False, end=False)
    assert r.calls[0][0]["packets"] == want.calls[0][0]["packets"] and len(want.calls[0][0]["packets"]) > 0
    assert all(c["packets"] == [] for c in r.calls[0][1:])


def test_strict_junk_with_nothing_chosen():
    """the one deviation from the file-side rule, which drops an unchosen tail"""
    sk = SEL.foreign("skeleton", 71, 1)
    junk = b"\x00" * 40
    assert SEL.model(sk[0] + junk)[0] == b""
    r = X.StrictRun("host", [sk[0] + junk, junk, sk[0] + junk[:26], b"OggS\x01" + junk], [[], [], [], []], end=False)
    assert [c[0]["status"] for c in r.calls] == [EOGG, EOGG, 0, EOGG]
    assert r.calls[2][0]["pending"] == 26
    # ... and the same junk behind a chosen stream
    m = X.tiny()[0]
    r = X.StrictRun("host", [m + junk], [[len(m)]], end=False)
    assert [c["status"] for c in r.calls[0]] == [0, EOGG]


def test_strict_end_without_a_vorbis_stream():
    m = X.corpus()["no vorbis at all"]
    r = X.StrictRun("host", [m], [[len(m)]])
    assert [c["status"] for c in r.calls[0]] == [0, EOGG] and r.calls[0][0]["consumed"] == len(m)


def test_strict_foreign_page_with_a_wrong_crc_is_stepped_over():
    m = X.tiny()[0]
    k = next(k for k, (p, n, kept, head) in enumerate(X.walk(m)) if not kept and not head and n > 40)
    bad = X.flip_page(m, k)
    cuts = X.random_cuts(m, 7)
    got, want = X.StrictRun("host", [bad], [cuts]), X.StrictRun("host", [m], [cuts])
    assert got.calls == want.calls and got.calls[0][-1]["status"] == 0


def test_strict_kept_page_with_a_wrong_crc():
    """VBM_EOGG, the packets in front of the page delivered in the same call: the second walk, with foreign pages between
    the records"""
    m = X.tiny()[0]
    pages = X.walk(m)
    kept = [k for k, pg in enumerate(pages) if pg[2]]
    k = kept[-2]
    assert any(not pages[j][2] for j in range(kept[2], k))
    bad = X.flip_page(m, k)
    r = X.StrictRun("host", [bad, bad], [[], [pages[kept[2]][0]]], end=False)
    upto = X.vorbis_only(m)[:X.map_cut(m, pages[k][0])]
    want = X.StrictRun("host", [upto], [[]], multiplexed=False, end=False)
    assert r.calls[0][0]["status"] == EOGG and r.calls[0][0]["packets"] == want.calls[0][0]["packets"] != []
    assert r.calls[1][1]["status"] == EOGG
    assert r.calls[1][0]["packets"] + r.calls[1][1]["packets"] == want.calls[0][0]["packets"]


# ---- resync mode -------------------------------------------------------------------------------------------------------

def test_resync_foreign_bos_page_while_a_link_is_open():
    """it does not close the link, drop its open packet or mark a gap; the Vorbis bos page behind it does all three"""
    m, v = X.tiny()
    pages = X.walk(m)
    kept = [k for k, pg in enumerate(pages) if pg[2]]
    # in front of a kept page that continues a packet
    k = next(k for k in kept if m[pages[k][0] + 5] & 1)
    at = pages[k][0]
    fb = SEL.foreign("theora", 777, 5)[0]
    second = SEL._cat(SEL.vorbis_pages(4))
    blob = m[:at] + fb + second                   # the mount moves on to its next group while a packet of link 0 is open
    run = X.resync_run("host", [blob], [[at, at + len(fb)]])
    X.check_resync_model(run, [blob], [[at, at + len(fb)]])
    calls = run.calls[0]
    assert (calls[1]["ignored"], calls[1]["link_started"], calls[1]["link"], calls[1]["gaps"]) == (1, 0, 0, 0)
    assert calls[1]["packets"] == [] and calls[1]["headers_ready"] == 1             # link 0 is still the slot's link
    assert calls[2]["link_started"] == 1 and calls[2]["link"] == 1
    got = RS.joined(calls)
    want = RS.Run("host", [v[:X.map_cut(m, at)] + second], [[]])
    assert got == RS.joined(want.calls[0]) and sorted(got) == [0, 1] and len(got[0]) > 0
    assert [p[3] for p in got[0]] == [0] * len(got[0]) and got[1][0][3] == 1     # one mark: the second link's first packet
    plain = RS.Run("host", [blob], [[at, at + len(fb)]])                             # without the flag it starts a link
    assert plain.calls[0][1]["link_started"] == 1 and plain.calls[0][1]["link"] == 1


def test_resync_damaged_foreign_page_is_skipped_bytes():
    m = X.tiny()[0]
    k = next(k for k, (p, n, kept, head) in enumerate(X.walk(m)) if not kept and not head and n > 40)
    n = X.walk(m)[k][1]
    bad = X.flip_page(m, k)
    got, want = X.resync_run("host", [bad], [[]]), X.resync_run("host", [m], [[]])
    X.check_resync_model(got, [bad], [[]])
    assert RS.joined(got.calls[0]) == RS.joined(want.calls[0])
    assert sum(c["skipped"] for c in got.calls[0]) == n and sum(c["skipped"] for c in want.calls[0]) == 0
    assert sum(c["ignored"] for c in got.calls[0]) == sum(c["ignored"] for c in want.calls[0]) - 1


def test_resync_damaged_vorbis_head_page():
    """that group never gets a link: its pages are ignored until the next group"""
    m = X.corpus()["three groups"]
    heads = [k for k, (p, n, kept, head) in enumerate(X.walk(m)) if kept and head]
    bad = X.flip_page(m, heads[1])
    run = X.resync_run("host", [bad], [X.random_cuts(bad, 5)])
    X.check_resync_model(run, [bad], [X.random_cuts(bad, 5)])
    links = SEL.vorbis_pages(4), SEL.vorbis_pages(2)
    want = RS.Run("host", [SEL._cat(links[0] + links[1])], [[]])
    assert RS.joined(run.calls[0]) == RS.joined(want.calls[0]) and sorted(run.headers[0]) == [0, 1]


def test_resync_damage_against_the_model():
    files = X.damaged_files()
    assert len(files) >= 9
    blobs = list(files.values())
    cuts = [X.random_cuts(b, 300 + i, 4) for i, b in enumerate(blobs)]
    X.check_resync_model(X.resync_run("host", blobs, cuts), blobs, cuts)


def test_resync_corpus_against_the_model():
    blobs = [X.corpus()[n] for n in X.small_names()] + [X.mid_join()]
    cuts = [X.random_cuts(b, 400 + i, 4) for i, b in enumerate(blobs)]
    run = X.check_resync_model(X.resync_run("host", blobs, cuts), blobs, cuts)
    joined = RS.joined(run.calls[-1])                                 # the mount joined mid-group: links 0 and 1 are
    want = RS.Run("host", [SEL._cat(SEL.vorbis_pages(3) + SEL.vorbis_pages(2))], [[]])          # groups 2 and 3
    assert joined == RS.joined(want.calls[0])


# ---- capacities --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("resync", [False, True])
def test_partial_foreign_page_and_max_page_carry(resync):
    rng = np.random.default_rng(8)
    m, v = X.tiny()
    big = SEL.sized_page(600, 9, 2000, rng)
    at = X.walk(m)[4][0]
    blob = m[:at] + big + m[at:]
    for carry, want in ((1999, 0), (1998, EBIG)):
        f = _feed(max_page_carry=carry, resync=resync, multiplexed=True)
        r1 = f.push([0], [blob[:at + 1999]])
        assert r1.status == [want] and int(r1.info[0]["pending"]) == (1999 if want == 0 else 0)
        r2 = f.push([0], [blob[at + 1999:]], end=True)
        assert r2.status == [want]
        if want == 0:                                                  # carried, then dropped
            ref = _feed(resync=resync)
            a, b = ref.push([0], [v[:X.map_cut(m, at)]]), ref.push([0], [v[X.map_cut(m, at):]], end=True)
            for g, w in ((r1, a), (r2, b)):
                assert g.payload.tobytes() == w.payload.tobytes() and g.offsets.tolist() == w.offsets.tolist()
                assert g.granulepos.tolist() == w.granulepos.tolist() and g.eos.tolist() == w.eos.tolist()
            ref.close()
        f.close()


@pytest.mark.parametrize("resync", [False, True])
def test_a_chunk_of_27_byte_foreign_pages_fills_no_record(resync):
    rng = np.random.default_rng(9)
    m = X.tiny()[0]
    at = X.walk(m)[4][0]
    small = b"".join(SEL.sized_page(600, 50 + k, 27, rng) for k in range(40))
    f = _feed(call=len(small) + len(m), resync=resync, multiplexed=True)
    r0 = f.push([0], [m[:at]])
    r = f.push([0], [small])
    assert r.status == [0] and int(r.info[0]["consumed"]) == len(small) and int(r.info[0]["packets"]) == 0
    if resync:
        assert int(r.events[0]["ignored_pages"]) == 40 and int(r.events[0]["left"]) == 0
    r2 = f.push([0], [m[at:]], end=True)
    ref = _feed(resync=resync, multiplexed=True)
    w0, w2 = ref.push([0], [m[:at]]), ref.push([0], [m[at:]], end=True)
    assert r2.status == [0] and r2.payload.tobytes() == w2.payload.tobytes() and r0.payload.tobytes() == w0.payload.tobytes()
    f.close(), ref.close()


# ---- slots -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("resync", [False, True])
def test_reset_makes_a_slot_fresh(resync):
    """after a reset the slot is in a new group with nothing chosen, and its first page counts as a head again"""
    m = X.tiny()[0]
    noflag = X.corpus()["first page without the flag, with the mark"]
    at = X.walk(m)[5][0]
    f = _feed(n=2, resync=resync, multiplexed=True)
    f.push([0, 1], [m[:at], m[:at]])
    f.reset([0])
    fresh = _feed(n=2, resync=resync, multiplexed=True)
    for blob in (noflag, m):
        a = f.push([0], [blob], end=True)
        b = fresh.push([0], [blob], end=True)
        assert a.info.tobytes() == b.info.tobytes() and a.payload.tobytes() == b.payload.tobytes()
        assert a.status == [0] and (resync or int(a.info[0]["packets"]) > 0)
        f.reset([0]), fresh.reset([0])
    r = f.push([1], [m[at:]], end=True)                               # the neighbour was not touched
    assert r.status == [0] and int(r.info[0]["packets"]) > 0
    f.close(), fresh.close()
