"""OggFeed(multiplexed=True) on the device (k_feed_walk<true>, k_feed_settle<true>, k_feed_resync_walk<true>): every call
equal to the host twin in its info and event structs, CSR and gap marks, through the calls that follow (which read the
committed slot state), the yardsticks of tests/ogg_feed_mux_cases.py on the device, and encoded audio between foreign
pages through the live loop of the README."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ogg_feed_mux_cases as X
from tests import ogg_feed_resync_cases as RS
from tests import ogg_select_cases as SEL
from tests.ogg_feed_mux_cases import EBIG, EINVAL, EOGG
from tests.signals import synth_signal
from tests.ogg_pages import split_pages

pytestmark = pytest.mark.gpu


def same_logs(dev, host):
    assert len(dev.log) == len(host.log)
    for k, (a, b) in enumerate(zip(dev.log, host.log)):
        assert a == b, (k, [i for i, (x, y) in enumerate(zip(a, b)) if x != y])
    assert dev.headers == host.headers
    return dev


def both_strict(blobs, cuts, **kw):
    return same_logs(X.StrictRun("device", blobs, cuts, **kw), X.StrictRun("host", blobs, cuts, **kw))


def both_resync(blobs, cuts, **kw):
    dev = same_logs(X.resync_run("device", blobs, cuts, **kw), X.resync_run("host", blobs, cuts, **kw))
    return dev


def test_flags(cuda):
    from vorbis_aotuv_lancer_amd._lib import lib
    for flags, want in ((4, 0), (5, 0), (8, EINVAL), (12, EINVAL), (6, EINVAL)):
        h = C.c_void_p()
        assert lib.vbm_ogg_feed_create2(C.byref(h), 2, 1000, 100, 100, 100, flags) == want, flags
        if want == 0:
            lib.vbm_ogg_feed_destroy(h)


# ---- the corpus, all slots in the same calls -----------------------------------------------------------------------------

def test_strict_corpus_random_cuts(cuda):
    blobs = list(X.corpus().values())
    cuts = [X.strict_cuts(b, X.random_cuts(b, 100 + i)) for i, b in enumerate(blobs)]
    dev = X.check_strict_equivalence("device", blobs, cuts)
    same_logs(dev, X.StrictRun("host", blobs, cuts))


def test_resync_corpus_random_cuts(cuda):
    blobs = list(X.corpus().values())
    cuts = [X.random_cuts(b, 200 + i) for i, b in enumerate(blobs)]
    dev = X.check_resync_equivalence("device", blobs, cuts)
    same_logs(dev, X.resync_run("host", blobs, cuts))


def test_resync_model_on_the_device(cuda):
    blobs = [X.corpus()[n] for n in X.small_names()] + [X.mid_join()]
    cuts = [X.random_cuts(b, 400 + i, 4) for i, b in enumerate(blobs)]
    X.check_resync_model(both_resync(blobs, cuts), blobs, cuts)


@pytest.mark.parametrize("resync", [False, True])
def test_every_cut_of_a_small_mount(cuda, resync):
    m = X.tiny()[0]
    cuts = [[c] for c in range(len(m) + 1)]
    if resync:
        dev = X.check_resync_equivalence("device", [m] * len(cuts), cuts)
        same_logs(dev, X.resync_run("host", [m] * len(cuts), cuts))
    else:
        dev = X.check_strict_equivalence("device", [m] * len(cuts), cuts)
        same_logs(dev, X.StrictRun("host", [m] * len(cuts), cuts))


@pytest.mark.parametrize("resync", [False, True])
def test_one_byte_per_call(cuda, resync):
    """the first 420 bytes (three head pages, the header packets, foreign pages, the first audio) one byte per call, then
    the rest"""
    m = X.tiny()[0]
    cuts = [list(range(1, 421))]
    assert sum(1 for p, n, _, _ in X.walk(m) if p + n <= 420) >= 6
    (both_resync if resync else both_strict)([m], cuts)


@pytest.mark.parametrize("resync", [False, True])
def test_cuts_in_foreign_pages_and_in_the_mark(cuda, resync):
    """... the head page of more than 244 segments among them: the wave walk's second round trip"""
    blobs, cuts = [], []
    for name in ("tiny", "three groups", "more than 244 segments in front of the mark"):
        m = X.corpus()[name]
        cs = [[c] for c in X.foreign_page_cuts(m) + X.mark_cuts(m)] + [sorted(set(X.foreign_page_cuts(m))), X.mark_cuts(m)]
        blobs += [m] * len(cs)
        cuts += cs
    if resync:
        dev = X.check_resync_equivalence("device", blobs, cuts)
        same_logs(dev, X.resync_run("host", blobs, cuts))
    else:
        dev = X.check_strict_equivalence("device", blobs, cuts)
        same_logs(dev, X.StrictRun("host", blobs, cuts))


# ---- damage --------------------------------------------------------------------------------------------------------------

def test_damage_resync(cuda):
    blobs = list(X.damaged_files().values())
    cuts = [X.random_cuts(b, 300 + i, 4) for i, b in enumerate(blobs)]
    X.check_resync_model(both_resync(blobs, cuts), blobs, cuts)


def test_damage_strict(cuda):
    """the strict feed on the same damaged mounts: whatever the twin decides, status and state through the later calls"""
    blobs = list(X.damaged_files().values())
    cuts = [X.random_cuts(b, 300 + i, 4) for i, b in enumerate(blobs)]
    dev = both_strict(blobs, cuts)
    assert {c[-1]["status"] for c in dev.calls} == {0, EOGG}


def test_strict_kept_page_with_a_wrong_crc(cuda):
    """k_feed_settle<true>: the second walk passes the foreign pages between the records as the first did"""
    m = X.tiny()[0]
    pages = X.walk(m)
    kept = [k for k, pg in enumerate(pages) if pg[2]]
    k = kept[-2]
    bad, foreign_bad = X.flip_page(m, k), X.flip_page(m, next(j for j, pg in enumerate(pages) if not pg[2] and j > 3))
    dev = both_strict([bad, bad, foreign_bad, m], [[], [pages[kept[2]][0]], [], []], end=False)
    assert [c[-1]["status"] for c in dev.calls] == [EOGG, EOGG, 0, 0]
    assert len(dev.calls[0][0]["packets"]) > 0 and dev.calls[2] == dev.calls[3]
    assert dev.calls[0][0]["packets"] == dev.calls[1][0]["packets"] + dev.calls[1][1]["packets"]


def test_strict_statuses(cuda):
    """a chain, junk with nothing chosen, no Vorbis stream at the end"""
    m = X.corpus()["two groups"]
    p, n = [(p, n) for p, n, kept, head in X.walk(m) if kept and head][1]
    sk = SEL.foreign("skeleton", 71, 1)
    none = X.corpus()["no vorbis at all"]
    dev = both_strict([m, sk[0] + b"\x00" * 40, none], [[p, p + 27, p + n - 1, p + n], [], [len(none)]])
    assert [c["status"] for c in dev.calls[0]] == [0, 0, 0, EOGG, EOGG]
    assert dev.calls[1][0]["status"] == EOGG and [c["status"] for c in dev.calls[2]] == [0, EOGG]


# ---- capacities and slots ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("resync", [False, True])
def test_partial_foreign_page_and_max_page_carry(cuda, resync):
    rng = np.random.default_rng(8)
    m = X.tiny()[0]
    at = X.walk(m)[4][0]
    blob = m[:at] + SEL.sized_page(600, 9, 2000, rng) + m[at:]
    small = b"".join(SEL.sized_page(600, 50 + k, 27, rng) for k in range(40))
    for carry, want in ((1999, 0), (1998, EBIG)):
        run = (both_resync if resync else both_strict)([blob, m[:at] + small + m[at:]], [[at + 1999], [at, at + len(small)]],
                                                       max_page_carry=carry)
        if resync:
            assert run.status[0] == want and run.status[1] == 0
            assert run.calls[1][1]["ignored"] == 40 and run.calls[1][1]["packets"] == []
        else:
            assert run.calls[0][-1]["status"] == want and run.calls[1][-1]["status"] == 0


@pytest.mark.parametrize("resync", [False, True])
def test_reset_makes_a_slot_fresh(cuda, resync):
    import vorbis_aotuv_lancer_amd as v
    m = X.tiny()[0]
    noflag = X.corpus()["first page without the flag, with the mark"]
    at = X.walk(m)[5][0]
    logs = []
    for host in (False, True):
        f = v.OggFeed(2, 1 << 16, host=host, resync=resync, multiplexed=True, max_packet_bytes=X.BIG, header_cap=X.BIG)
        log = []
        f.push([0, 1], [m[:at], m[:at]])
        f.reset([0])
        for blob in (noflag, m):
            r = f.push([0], [blob], end=True)
            log.append((r.info.tobytes(), RS._np(r.payload).tobytes(), RS._np(r.offsets).tobytes()))
            f.reset([0])
        r = f.push([1], [m[at:]], end=True)
        assert r.status == [0] and int(r.info[0]["packets"]) > 0
        log.append((r.info.tobytes(), RS._np(r.payload).tobytes(), RS._np(r.offsets).tobytes()))
        logs.append(log)
        f.close()
    assert logs[0] == logs[1]


def test_the_default_did_not_move(cuda):
    m = X.corpus()["skeleton first"]
    r = both_strict([m], [[]], multiplexed=False)
    assert r.calls[0][0]["status"] == EOGG
    dev, host = RS.Run("device", [m], [[]]), RS.Run("host", [m], [[]])
    assert dev.log == host.log and dev.calls[0][0]["link_started"] == 1 and dev.calls[0][0]["left"] > 0


# ---- end to end: encoded audio between foreign pages ----------------------------------------------------------------------

def _p(blob):
    return [bytes(p) for p in split_pages(blob)]


@pytest.fixture(scope="module")
def mounts(cuda):
    """two mounts of different header classes, the first chained across both: (multiplexed, Vorbis-only)"""
    import vorbis_aotuv_lancer_amd as v
    st = v.encode_ogg([synth_signal(2, 44100, 15000, seed=70)], 44100, quality=0.5, serialnos=[31])[0]
    mono = v.encode_ogg([synth_signal(1, 8000, n, seed=80 + i) for i, n in enumerate((3000, 4000))], 8000, quality=0.5,
                        serialnos=[41, 42])
    sk = SEL.foreign("skeleton", 71, 1, sizes=(80, 600, 80))
    g1 = [sk[0], _p(st)[0]] + SEL.interleave([sk[1:], _p(st)[1:]], 3)
    g2 = SEL.interleave([SEL.foreign("theora", 71, 4), _p(mono[0]), SEL.foreign("opus", 31, 6)], 5)
    other = SEL.interleave([_p(mono[1]), SEL.foreign("theora", 73, 7, sizes=(40, 3000, 9, 700, 5000), max_segs=9)], 8)
    muxed = [SEL._cat(g1 + g2), SEL._cat(other)]
    plain = [st + mono[0], mono[1]]
    for m, w in zip(muxed, plain):
        assert X.vorbis_only(m) == w
    return muxed, plain


def _live_loop(blobs, cuts, multiplexed):
    """the README's loop -> per slot, per link: the PCM of all calls back to back"""
    import vorbis_aotuv_lancer_amd as v
    n = len(blobs)
    feed = v.OggFeed(n, max_call_bytes=n * 65536, max_page_carry=65307, resync=True, multiplexed=multiplexed)
    md = v.MixedDecoder(n, 2048, max_classes=4, max_channels=2, max_blocksize=2048)
    link_of = np.full(n, -1)
    out, ignored = [[] for _ in range(n)], 0
    edges = [[0] + list(c) + [len(b)] for b, c in zip(blobs, cuts)]
    for k in range(len(edges[0]) - 1):
        chunks = [b[e[k]:e[k + 1]] for b, e in zip(blobs, edges)]
        for r in feed.push_all(np.arange(n), chunks, end=k == len(edges[0]) - 2):
            assert not any(r.status)
            ignored += int(r.events["ignored_pages"].sum())
            ready = (r.info["headers_ready"] != 0) & (r.link != link_of[r.ids])
            for i in np.flatnonzero(ready):
                md.bind([r.ids[i]], [md.class_for(feed.headers(r.ids[i]))])
                link_of[r.ids[i]] = r.link[i]
                out[r.ids[i]].append([])
            live = r.counts > 0
            if not live.any():
                continue
            pcm, ns, _, st = md.synthesis_runs(r.ids[live], r.counts[live], r.payload, r.offsets, granulepos=r.granulepos,
                                               eos=r.eos, gap=r.gap)
            assert not st.cpu().numpy().any()
            ch = md.channels_of(r.ids[live])
            for row, slot in enumerate(r.ids[live].tolist()):
                out[slot][-1].append(pcm[row, :ch[row], :int(ns[row])].cpu())
    feed.close()
    md.close()
    return [[torch.cat(link, dim=1) for link in slot] for slot in out], ignored


def test_live_loop_on_multiplexed_mounts(cuda, mounts):
    muxed, plain = mounts
    rng = np.random.default_rng(17)
    cuts = [sorted(int(x) for x in rng.integers(0, len(m) + 1, 7)) for m in muxed]
    got, ignored = _live_loop(muxed, cuts, True)
    want, none = _live_loop(plain, [[X.map_cut(m, c) for c in cs] for m, cs in zip(muxed, cuts)], False)
    assert [len(s) for s in got] == [2, 1] and none == 0
    assert ignored == sum(X.foreign_before(m, len(m)) for m in muxed) > 10
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for a, b in zip(g, w):
            assert a.shape == b.shape and a.shape[1] > 1000 and torch.equal(a, b)
    # the flag changes nothing on the Vorbis-only mounts
    same, none = _live_loop(plain, [[len(p) // 3] for p in plain], True)
    assert none == 0 and all(torch.equal(a, b) for g, w in zip(same, want) for a, b in zip(g, w))


def test_two_feeds_on_two_streams(cuda, mounts):
    """two multiplexed resync feeds on two streams, three calls each enqueued with no host wait in between: every output
    equals the host twin's"""
    from vorbis_aotuv_lancer_amd._lib import lib
    from vorbis_aotuv_lancer_amd.stream import FEED_EVENTS, FEED_INFO
    muxed, _ = mounts
    work = []
    for blobs in ([muxed[0], muxed[1]], [muxed[1], X.tiny()[0], muxed[0]]):
        cuts = [[len(b) // 3, 2 * len(b) // 3] for b in blobs]
        host = X.resync_run("host", blobs, cuts)              # three pushes, and one more for every part that came back
        feed = RS.make_feed("device", len(blobs), max(len(raw) for _, raw, _, _ in host.inputs), multiplexed=True)
        bufs = []
        for (ids, raw, off, end), want in zip(host.inputs, host.log):
            n, P, B = len(ids), len(want[5]) // 8, len(want[3])
            bufs.append(dict(ids=ids, off=off, end=end, data=torch.from_numpy(raw).cuda(), P=P, B=B, want=want,
                             meta=torch.zeros(16 + n * (FEED_INFO.itemsize + FEED_EVENTS.itemsize), dtype=torch.uint8, device="cuda"),
                             payload=torch.zeros(B, dtype=torch.uint8, device="cuda"),
                             offsets=torch.zeros(P + 1, dtype=torch.int64, device="cuda"),
                             granulepos=torch.zeros(P, dtype=torch.int64, device="cuda"),
                             eos=torch.zeros(P, dtype=torch.uint8, device="cuda"),
                             gap=torch.zeros(P, dtype=torch.uint8, device="cuda")))
        work.append(dict(feed=feed, bufs=bufs))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for j in range(max(len(w["bufs"]) for w in work)):
        for w, q in zip(work, streams):
            if j >= len(w["bufs"]):
                continue
            b, h, s = w["bufs"][j], w["feed"]._h, C.c_void_p(q.cuda_stream)
            n, m = len(b["ids"]), b["meta"].data_ptr()
            assert lib.vbm_ogg_feed_scan(h, n, b["ids"].ctypes.data, b["data"].data_ptr(), b["off"].ctypes.data,
                                         b["end"].ctypes.data, m + 16, m, s) == 0
            assert lib.vbm_ogg_feed_scan_events(h, m + 16 + n * FEED_INFO.itemsize, s) == 0
            assert lib.vbm_ogg_feed_fill_gaps(h, b["payload"].data_ptr(), b["B"], b["offsets"].data_ptr(),
                                              b["granulepos"].data_ptr(), b["eos"].data_ptr(), b["gap"].data_ptr(), b["P"],
                                              s) == 0
    torch.cuda.synchronize()
    for w in work:
        assert len(w["bufs"]) >= 3
        for k, b in enumerate(w["bufs"]):
            n, meta = len(b["ids"]), b["meta"].cpu().numpy()
            ni = n * FEED_INFO.itemsize
            got = (b["ids"].tobytes(), meta[16:16 + ni].tobytes(), meta[16 + ni:].tobytes()) + \
                tuple(b[x].cpu().numpy().tobytes() for x in ("payload", "offsets", "granulepos", "eos", "gap"))
            assert got == b["want"], k
            assert meta[:16].view(np.int64).tolist() == [b["P"], b["B"]]
        w["feed"].close()
