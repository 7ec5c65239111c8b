"""Shared by test_ogg_feed_mux_cpu.py and test_ogg_feed_mux_gpu.py: multiplexed mounts for OggFeed(multiplexed=True),
built from the corpus of the file-side selection (tests/ogg_select_cases.py), and the three yardsticks.

1. Equivalence on undamaged input.  With V = the kept bytes of M by the rule of csrc/ogg_select.h (ogg_select_cases.model,
   pinned against select_vorbis_stream) and map_cut(M, c) = the bytes of V in front of byte c of M, call k of the flagged
   feed on M cut at c_k equals call k of the unflagged feed on V cut at map_cut(M, c_k) in everything but pending,
   consumed, skipped_bytes and ignored_pages; ignored_pages exceeds the unflagged feed's by the foreign pages the call
   passed.  One deviation is inherent in the rule and pinned by a test of its own: a strict feed judges a head page that
   has to show the mark once it is whole, so the VBM_EOGG of a chain comes with the last byte of the second group's
   Vorbis head page and not with its 27th; strict_cuts moves cuts that fall between the two to the page's end.
2. Resync with damage: MuxSlot, the byte-serial model of tests/ogg_resync_model.py with the group rule in front of its
   rule 2.
3. The device against the host twin: drivers here return logs of everything a call returned, as bytes."""
import functools
import struct

import numpy as np

from tests import ogg_chain_cases as CH
from tests import ogg_feed_resync_cases as RS
from tests import ogg_pages as PG
from tests import ogg_resync_model as M
from tests import ogg_select_cases as SEL
from tests.ogg_pages import corruptions, random_bytes

EOGG, EBIG, EINVAL = -1002, -1003, -131
MUX, RESYNC = 4, 1
BIG = RS.BIG


# ---- pages of a multiplexed file by the rule, and the cut mapping -----------------------------------------------------

def walk(data):
    """-> [(pos, len, kept, head)] of every page of the undamaged file `data`, by the rule of csrc/ogg_select.h"""
    return list(_walk(bytes(data)))


@functools.lru_cache(maxsize=None)
def _walk(data):
    out, pos, state = [], 0, PG.GROUP_START
    for p in PG.parse(data, 0, len(data)):
        head = bool(p.flags & 2) or p.pos == 0
        state, _ = PG.group_step(state, head, p.serial, PG.body7(data, p))
        out.append((p.pos, p.size, state[1] and p.serial == state[2], head))
        pos = p.pos + p.size
    assert pos == len(data), "the equivalence corpus holds whole pages only"
    return tuple(out)


def vorbis_only(data):
    return SEL.model(data)[0]


def map_cut(data, c):
    """byte position c of M -> the position in V: the kept bytes of the whole pages in front of c, and, if c lies inside
    a kept page, the part of that page in front of c"""
    return sum(min(max(c - src, 0), n) for src, n, _ in SEL.model(data)[2])


def foreign_before(data, c):
    """foreign pages of M that end at or in front of byte c"""
    return sum(1 for p, n, kept, _ in walk(data) if not kept and p + n <= c)


def strict_cuts(data, cuts):
    """cuts for the strict equivalence: one that falls behind the 27th byte of a kept head page after the first kept
    page, with the page not whole, moves to the page's end (see the head of this file)"""
    late = [(p, n) for p, n, kept, head in walk(data) if kept and head][1:]
    out = []
    for c in cuts:
        for p, n in late:
            if p + 27 <= c < p + n:
                c = p + n
        out.append(c)
    return sorted(out)


def random_cuts(data, seed, k=6):
    rng = np.random.default_rng(seed)
    return sorted(int(x) for x in rng.integers(0, len(data) + 1, k))


def foreign_page_cuts(m):
    """inside a foreign page's header, its lacing table and its body, and at its two ends; the page has a body"""
    p, n = next((p, n) for p, n, kept, head in walk(m) if not kept and not head and m[p + 26] >= 1 and n > 40)
    nseg = m[p + 26]
    return [p, p + 1, p + 26, p + 27, p + 27 + nseg - 1, p + 27 + nseg, p + 27 + nseg + 1, p + n - 1, p + n]


def mark_cuts(m):
    p, nseg = next((p, m[p + 26]) for p, n, kept, head in walk(m) if kept and head)
    return [p + 27 + nseg + k for k in range(1, 7)]


# ---- corpus -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny():
    """-> (M, V): a Vorbis-like stream of a few hundred bytes (a head page with the mark, two more header packets, audio
    packets of tens of bytes, one continued over a page) between the pages of two foreign streams, Skeleton-like first"""
    rng = np.random.default_rng(41)
    rb = functools.partial(random_bytes, rng)
    pk = [PG.MARK + rb(23), rb(11), rb(14)] + [rb(n) for n in (20, 0, 31, 255, 9, 300, 17)]
    v = PG.lay(pk, 500, max_segs=2)
    sk = PG.lay([b"fishead\0" + rb(20), rb(12), rb(40)], 600, max_segs=1)
    th = PG.lay([b"\x80theora" + rb(9), rb(260), b""], 601, max_segs=1)
    other = [p for pair in zip(sk[1:], th[1:]) for p in pair]   # behind the heads: a Vorbis page, a foreign one, and so on
    assert len(other) == 4 and len(v) >= 7
    rest = [p for pair in zip(v[1:], other) for p in pair] + v[1 + len(other):]
    m = SEL._cat([sk[0], v[0], th[0]] + rest)
    RS.assert_no_stray_capture(m)
    assert 600 < len(m) < 1500 and vorbis_only(m) == SEL._cat(v)
    return m, SEL._cat(v)


@functools.lru_cache(maxsize=None)
def many_segments():
    """a Vorbis head page with 250 segments of no bytes in front of the segment that holds the mark: on the device the
    mark lies behind the 256 bytes the header round trip brings"""
    v = SEL.vorbis_pages(4)
    h = v[0]
    body = h[27 + h[26]:]
    assert h[26] == 1 and body[:7] == PG.MARK
    head = PG.page(struct.unpack_from("<I", h, 14)[0], 0, [0] * 250 + [len(body)], body, flags=2)
    sk = SEL.foreign("skeleton", 93, 51, sizes=(30, 200))
    return SEL._cat([sk[0], head] + PG.interleave([sk[1:], v[1:]], 52))


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> undamaged multiplexed mount (whole pages)"""
    out = {name: m for name, m, _ in SEL.singles()}
    e = SEL.case8()
    for name in ("head page of no segments", "head page with a body of 6", "body of 7, one byte wrong",
                 "head page with a body of exactly 7", "first page without the flag, with the mark"):
        out[name] = e[name]
    out["more than 244 segments in front of the mark"] = many_segments()
    out["tiny"] = tiny()[0]
    out["plain stream"] = SEL.case7()["link 0"]
    out["plain chain"] = CH.chains()["2 links"][0]
    out["no vorbis at all"] = SEL.case6()["two foreign streams"]
    for m in out.values():
        walk(m)
    return out


def small_names():
    """the corpus without its one large file, for what runs through the Python model"""
    return [n for n in corpus() if n != "video-like"]


def mid_join():
    """a mount joined inside a foreign page of its first group: the listener's first bytes are the rest of that page"""
    m = SEL.case5()["three groups"][0]
    p, n = next((p, n) for p, n, kept, head in walk(m) if not kept and not head and n > 60)
    return m[p + n // 2:]


# ---- the resync model with the group rule --------------------------------------------------------------------------------

class MuxSlot(M.Slot):
    """ogg_resync_model.Slot with the group rule between its rules 1 and 2.  The rule runs on a copy of its state, which
    is committed once the page goes by: a page the call stops at is judged again by the next.  tracked: the serial
    number the product's slot tracks (none, 0, for a link that went bad at its first page)."""

    def __init__(self):
        super().__init__()
        self.in_heads, self.chosen, self.tracked = PG.GROUP_START
        self.met = False              # a page has gone by: until then any page is a head page
        self.judged = None            # (in_heads, chosen) behind the page in hand

    def foreign(self, page, nseg, bos, serial):
        state, _ = PG.group_step((self.in_heads, self.chosen, self.tracked), bos or not self.met, serial,
                                 page[27 + nseg:27 + nseg + 7])
        self.judged = state[:2]
        if state[1] and serial == state[2]:
            return False                                   # the page is kept: rule 2 judges it
        self.passed()
        return True

    def passed(self):
        (self.in_heads, self.chosen), self.met = self.judged, True

    def link_started(self):
        self.tracked = 0

    def page_taken(self, serial):
        self.tracked = serial


def model_run(data, cuts=(), end=True):
    return M.run(data, cuts, end, slot=MuxSlot())


# ---- drivers -------------------------------------------------------------------------------------------------------------

def resync_run(impl, blobs, cuts, multiplexed=True, end=True, **kw):
    """ogg_feed_resync_cases.Run over a resync feed, multiplexed or not"""
    if multiplexed:
        kw["multiplexed"] = True
    return RS.Run(impl, blobs, cuts, end, **kw)


def check_resync_model(run, blobs, cuts, end=True):
    """every call of every slot equals MuxSlot's, and so do the headers of every link"""
    return RS.check_against_model(run, blobs, cuts, end, model=MuxSlot)


def check_resync_equivalence(impl, blobs, cuts, **kw):
    """yardstick 1 for the resync mode -> the flagged feed's Run"""
    plain = [vorbis_only(b) for b in blobs]
    pcuts = [[map_cut(b, c) for c in cs] for b, cs in zip(blobs, cuts)]
    got = resync_run(impl, blobs, cuts, **kw)
    want = resync_run(impl, plain, pcuts, multiplexed=False, **kw)
    for s, b in enumerate(blobs):
        edges = list(cuts[s]) + [len(b)]
        assert len(got.calls[s]) == len(want.calls[s]), (s, len(got.calls[s]), len(want.calls[s]))
        k = 0                                                      # the piece a call belongs to
        for j, (g, w) in enumerate(zip(got.calls[s], want.calls[s])):
            for name in ("packets", "link", "link_started", "link_bad", "gaps", "headers_ready"):
                assert g[name] == w[name], (s, j, name)
            reached = edges[k] - g["left"]                         # `left`, mapped: both feeds stopped at the same page
            assert map_cut(b, reached) == map_cut(b, edges[k]) - w["left"], (s, j)
            assert g["ignored"] >= w["ignored"], (s, j)            # (a foreign page counts in the call that completes it)
            if g["left"] == 0:
                k = min(k + 1, len(edges) - 1)
        assert sum(g["ignored"] for g in got.calls[s]) == \
            sum(w["ignored"] for w in want.calls[s]) + foreign_before(b, len(b)), s
        assert got.headers[s] == want.headers[s] and got.status[s] == want.status[s] == 0, s
    return got


class StrictRun:
    """blobs[s] goes to slot s of a strict feed cut at cuts[s], piece k of every stream that has one in call k, `end` with
    each stream's last piece.  .calls[s]: per call a dict of what the slot got; .log: everything every call returned."""

    def __init__(self, impl, blobs, cuts, multiplexed=True, end=True, feed=None, **kw):
        import vorbis_aotuv_lancer_amd as v
        n = len(blobs)
        edges = [[0] + list(c) + [len(b)] for b, c in zip(blobs, cuts)]
        rounds = max(len(e) - 1 for e in edges)
        biggest = max(sum(e[k + 1] - e[k] for e in edges if k < len(e) - 1) for k in range(rounds))
        kw.setdefault("max_packet_bytes", BIG)
        kw.setdefault("header_cap", BIG)
        if multiplexed:                                            # (not named otherwise: the default feed as it always was made)
            kw["multiplexed"] = True
        self.feed = feed or v.OggFeed(n, max(1, biggest), host=impl == "host", **kw)
        self.calls, self.log, self.headers = [[] for _ in blobs], [], [None] * n
        for k in range(rounds):
            who = [s for s in range(n) if k < len(edges[s]) - 1]
            parts = [bytes(blobs[s][edges[s][k]:edges[s][k + 1]]) for s in who]
            self.push(who, parts, [int(end and k == len(edges[s]) - 2) for s in who])
        if feed is None:
            self.feed.close()

    def push(self, who, parts, flags):
        r = self.feed.push(who, parts, np.array(flags, np.uint8))
        pay, offs, gp, eos = (RS._np(x) for x in (r.payload, r.offsets, r.granulepos, r.eos))
        self.log.append((r.ids.tobytes(), r.info.tobytes(), pay.tobytes(), offs.tobytes(), gp.tobytes(), eos.tobytes()))
        for i, s in enumerate(who):
            fi = r.info[i]
            base, n = int(fi["packet_base"]), int(fi["packets"])
            pk = [(pay[int(offs[base + k]):int(offs[base + k + 1])].tobytes(), int(gp[base + k]), int(eos[base + k]))
                  for k in range(n)]
            assert int(fi["payload_bytes"]) == int(offs[base + n] - offs[base])
            self.calls[s].append({"packets": pk, "status": int(fi["status"]), "headers_ready": int(fi["headers_ready"]),
                                  "header_bytes": fi["header_bytes"].tolist(), "serialno": int(fi["serialno"]),
                                  "pending": int(fi["pending"]), "consumed": int(fi["consumed"])})
            if fi["headers_ready"] and self.headers[s] is None:
                self.headers[s] = self.feed.headers(s)
        return r


SAME_STRICT = ("packets", "status", "headers_ready", "header_bytes", "serialno")


def check_strict_equivalence(impl, blobs, cuts, **kw):
    """yardstick 1 for the strict mode (cuts: through strict_cuts) -> the flagged feed's StrictRun"""
    plain = [vorbis_only(b) for b in blobs]
    pcuts = [[map_cut(b, c) for c in cs] for b, cs in zip(blobs, cuts)]
    got = StrictRun(impl, blobs, cuts, **kw)
    want = StrictRun(impl, plain, pcuts, multiplexed=False, **kw)
    for s in range(len(blobs)):
        assert len(got.calls[s]) == len(want.calls[s])
        for j, (g, w) in enumerate(zip(got.calls[s], want.calls[s])):
            for name in SAME_STRICT:
                assert g[name] == w[name], (s, j, name, g[name] if name != "packets" else len(g[name]),
                                            w[name] if name != "packets" else len(w[name]))
        assert got.headers[s] == want.headers[s], s
    return got


def damaged_files():
    """the corruptions variants of three small multiplexed files"""
    out = {}
    for src in ("skeleton first", "three groups", "two vorbis streams behind a foreign one"):
        for name, bad in corruptions(corpus()[src]).items():
            out[f"{src}: {name}"] = bad
    return out


def flip_page(data, k, at=None):
    """page k of the undamaged file with one body (or header, at < 27) byte flipped: its CRC no longer holds"""
    p, n, _, _ = walk(data)[k]
    b = bytearray(data)
    b[p + (n - 1 if at is None else at)] ^= 0x20
    return bytes(b)
