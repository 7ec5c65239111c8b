"""Shared by test_ogg_feed_resync_cpu.py, test_ogg_feed_resync_gpu.py and test_decode_gaps_gpu.py: damaged and chained
inputs for the resync feed, a driver that pushes several streams per call through OggFeed.push_all (host twin or device)
and logs every call, and the comparison with the byte-serial model (tests/ogg_resync_model.py)."""
import functools
import struct

import numpy as np

from tests import ogg_resync_model as M
from tests.ogg_demux_batch import directed, mixed, single
from tests.ogg_pages import pack, random_bytes, split_pages

BIG = 1 << 17
CHUNKS = (26, 27, 28, 255, 256, 4096)
EBIG, EINVAL, ECAP = -1003, -131, 1


def pages(blob):
    return split_pages(blob, as_bytes=True)


def join(ps):
    return b"".join(bytes(p) for p in ps)


def cuts_every(n, step):
    return list(range(step, n, step))


# ---- corpora -----------------------------------------------------------------------------------------------------------

def assert_no_stray_capture(blob):
    """no page body of the input holds "OggS" away from a page start: damage tests rely on it"""
    at, starts = 0, set()
    for p in split_pages(blob):
        starts.add(at)
        at += len(p)
    k = blob.find(b"OggS")
    while k >= 0:
        assert k in starts, f"OggS inside a page at byte {k}"
        k = blob.find(b"OggS", k + 1)


@functools.lru_cache(maxsize=None)
def good_files():
    """(name, blob): the undamaged single-link files of the directed and mixed corpora"""
    out = [(n, b) for n, b in directed() + mixed() if b and single(b) is not None]
    assert len(out) >= 8
    return out


def _mux(packets, serialno, flush):
    """headers on their own pages, then the packets; flush(k): packet k ends its page"""
    import vorbis_aotuv_lancer_amd as v
    os_, out = v.OggStream(serialno), []
    for h in v.header_packets(v.Setup(1, 44100, 0.1)):
        os_.packetin(h, 0)
    out += os_.pages(flush=True)
    for k, p in enumerate(packets):
        os_.packetin(p, 64 * (k + 1), k == len(packets) - 1)
        out += os_.pages(flush=flush(k))
    out += os_.pages(flush=True)
    os_.close()
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def paged_six():
    """the six packets of six_packet_file, one per page: six audio pages"""
    rng = np.random.default_rng(9)
    pk = [random_bytes(rng, n) for n in (300, 255, 1, 600, 0, 2000)]
    blob = _mux(pk, 31, lambda k: True)
    assert len(audio_pages(blob)) == 6
    assert_no_stray_capture(blob)
    return blob


@functools.lru_cache(maxsize=None)
def long_file():
    """a few dozen pages of one to three packets; two packets of 70000 bytes in a row, so that one page ends a spanning
    packet and begins the next"""
    rng = np.random.default_rng(5)
    sizes = [int(x) for x in rng.integers(1, 700, 60)]
    sizes[7], sizes[8], sizes[20], sizes[21] = 70000, 70000, 255 * 3, 0
    pk = [random_bytes(rng, n) for n in sizes]
    blob = _mux(pk, 4242, lambda k: k % 3 == 2 and k not in (7, 8))
    assert 20 <= len(pages(blob)) <= 60
    assert_no_stray_capture(blob)
    return blob


def audio_pages(blob):
    """the numbers of the pages on which no header packet lies"""
    done, out = 0, []
    for k, p in enumerate(split_pages(blob)):
        if done >= 3:
            out.append(k)
        done += sum(1 for lv in p[27:27 + p[26]] if lv < 255)
    return out


def packets_by_page(blob):
    """-> [(first page, last page, bytes, granulepos, eos)] of every audio packet, by a lacing walk of its own"""
    out, open_, first, done = [], None, 0, 0
    for k, p in enumerate(split_pages(blob)):
        nseg = p[26]
        body, ends = bytes(p[27 + nseg:]), [i for i in range(nseg) if p[27 + i] < 255]
        for i in range(nseg):
            if open_ is None:
                open_, first = b"", k
            lv = p[27 + i]
            open_, body = open_ + body[:lv], body[lv:]
            if lv < 255:
                last = i == ends[-1]
                if done >= 3:
                    out.append((first, k, open_, struct.unpack_from("<q", p, 6)[0] if last else -1,
                                int(bool(p[5] & 4) and last)))
                done, open_ = done + 1, None
    return out


def without_pages(blob, drop):
    return join(p for k, p in enumerate(pages(blob)) if k not in drop)


def survivors(blob, drop):
    """what a removal must leave: the packets that lie wholly on the remaining pages, the first behind the hole marked"""
    out = [[pk, gp, eos, 0, first] for first, last, pk, gp, eos in packets_by_page(blob)
           if not any(first <= d <= last for d in drop)]
    behind = [r for r in out if r[4] > max(drop)]
    if behind:
        behind[0][3] = 1
    return [tuple(r[:4]) for r in out]


def flip(blob, page, where):
    """one byte of page `page` flipped: where = 'header' (the granule position), 'lacing' or 'body'; None when the page
    has no such byte"""
    ps = [bytearray(p) for p in pages(blob)]
    p = ps[page]
    at = {"header": 7, "lacing": 27, "body": 27 + p[26] + (len(p) - 27 - p[26]) // 2}[where]
    if at >= len(p):
        return None                                  # a page without a body
    p[at] ^= 0x10
    return join(ps)


def false_capture_file():
    """One packet per page; the third packet's payload holds "OggS", version 0 and a lacing table whose body is all
    there.  The second audio page is removed and the third has lost its first 10 bytes (a listener who joins mid-page),
    so the walk searches through that page's body and meets the false header: a whole candidate with a bad CRC.
    -> (the damaged bytes, the packets that must come out, the bytes that must be skipped)"""
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(77)
    fake = b"OggS\0\0" + bytes(20) + b"\x02\x10\x08" + bytes(24)              # claims 27 + 2 + 24 bytes
    pk = [random_bytes(rng, n) for n in (200, 300)] + [b"ab" + fake + b"cd"] + \
         [random_bytes(rng, 150)]
    os_, out = v.OggStream(99), []
    for h in v.header_packets(v.Setup(1, 44100, 0.1)):
        os_.packetin(h, 0)
    out += os_.pages(flush=True)
    for k, p in enumerate(pk):
        os_.packetin(p, 100 * (k + 1), k == len(pk) - 1)
        out += os_.pages(flush=True)
    os_.close()
    ps = pages(b"".join(out))
    ap = audio_pages(b"".join(out))
    assert len(ap) == 4 and fake in ps[ap[2]]
    blob = join(ps[:ap[1]]) + ps[ap[2]][10:] + ps[ap[3]]
    return blob, [(pk[0], 100, 0, 0), (pk[3], 400, 1, 1)], len(ps[ap[2]]) - 10


@functools.lru_cache(maxsize=None)
def overclaim_file():
    """45 packets of 50 bytes, one per page of 78 bytes; the sixth audio page is cut down to a header that claims 2550
    body bytes and has 20 (a reconnect mid-page).  Everything behind it is carried until the claim is filled; then its
    CRC fails and the walk meets more whole pages in the tail than a small chunk has page records for.
    -> (the damaged bytes, the packets that must come out)"""
    rng = np.random.default_rng(12)
    blob = _mux([random_bytes(rng, 50) for _ in range(45)], 808, lambda k: True)
    ps, ap = pages(blob), audio_pages(blob)
    assert len(ap) == 45 and all(len(ps[k]) == 78 for k in ap)
    assert_no_stray_capture(blob)
    cut = ps[ap[5]][:26] + bytes([10]) + bytes([255] * 10) + bytes(range(20))
    return join(ps[:ap[5]]) + cut + join(ps[ap[6]:]), survivors(blob, {ap[5]})


@functools.lru_cache(maxsize=None)
def chain_files():
    """name -> chained file, from the chain corpus"""
    from tests import ogg_chain_cases as CH
    keep = ("2 links", "3 links", "three classes", "headers alone in the middle", "255 segments", "zero segments")
    return {k: CH.chains()[k][0] for k in keep}


# ---- driver ------------------------------------------------------------------------------------------------------------

def make_feed(impl, nslots, call_bytes, resync=True, **kw):
    import vorbis_aotuv_lancer_amd as v
    kw.setdefault("max_packet_bytes", BIG)
    kw.setdefault("header_cap", BIG)
    return v.OggFeed(nslots, max(1, call_bytes), host=impl == "host", resync=resync, **kw)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def entry_record(r, i):
    """list entry i of a FeedResult, in the form of the model's call record"""
    fi, ev = r.info[i], r.events[i]
    base, n = int(fi["packet_base"]), int(fi["packets"])
    offs, pay = _np(r.offsets)[base:base + n + 1], _np(r.payload)
    gp, eos, gap = _np(r.granulepos)[base:base + n], _np(r.eos)[base:base + n], _np(r.gap)[base:base + n]
    pk = [(pay[int(offs[k]):int(offs[k + 1])].tobytes(), int(gp[k]), int(eos[k]), int(gap[k])) for k in range(n)]
    assert int(fi["payload_bytes"]) == int(offs[n] - offs[0]) and int(fi["payload_base"]) == int(offs[0])
    return {"packets": pk, "link": int(ev["link"]), "link_started": int(ev["link_started"]), "link_bad": int(ev["link_bad"]),
            "gaps": int(ev["gaps"]), "skipped": int(ev["skipped_bytes"]), "ignored": int(ev["ignored_pages"]),
            "left": int(ev["left"]), "headers_ready": int(fi["headers_ready"])}


def log_entry(r):
    """everything a call returned, as bytes: for the device-against-twin comparison"""
    return (r.ids.tobytes(), r.info.tobytes(), r.events.tobytes(), _np(r.payload).tobytes(), _np(r.offsets).tobytes(),
            _np(r.granulepos).tobytes(), _np(r.eos).tobytes(), _np(r.gap).tobytes())


class Run:
    """blobs[s] goes to slot slots[s], cut at cuts[s]; round k pushes piece k of every stream that has one, in one call
    (and push_all pushes what is left).  .calls[s]: the slot's call records; .headers[s]: {link: [3 packets]};
    .log: every FeedResult as bytes."""

    def __init__(self, impl, blobs, cuts, end=True, slots=None, first=0, feed=None, nslots=None, **kw):
        n = len(blobs)
        self.slots = list(range(n)) if slots is None else list(slots)
        edges = [[0] + list(c) + [len(b)] for b, c in zip(blobs, cuts)]
        rounds = max(len(e) - 1 for e in edges)
        biggest = max(sum(e[k + 1] - e[k] for e in edges if k < len(e) - 1) for k in range(rounds))
        self.feed = feed or make_feed(impl, nslots or max(self.slots) + 1, biggest + first, **kw)
        self.calls, self.headers, self.log, self.status = [[] for _ in blobs], [{} for _ in blobs], [], [0] * n
        self.inputs = []
        for k in range(rounds):
            who = [s for s in range(n) if k < len(edges[s]) - 1]
            parts = [bytes(blobs[s][edges[s][k]:edges[s][k + 1]]) for s in who]
            flags = [int(end and k == len(edges[s]) - 2) for s in who]
            self.push(who, parts, flags, first)
        if feed is None:
            self.feed.close()

    def push(self, who, parts, flags, first=0):
        raw, off = pack(parts, first)
        if not self.feed.host:
            import torch
            raw = torch.from_numpy(raw.copy()).cuda()
        slot_of = {self.slots[s]: s for s in who}
        inner = self.feed.push

        def recorded(ids, chunks, end=False, offsets=None):      # the arguments of every push, the pushes of left parts too
            self.inputs.append((np.array(ids, np.int32), _np(chunks).copy(), np.array(offsets, np.int64),
                                np.array(end, np.uint8)))
            return inner(ids, chunks, end, offsets)

        self.feed.push = recorded
        try:
            self._push_all(who, raw, flags, off, slot_of)
        finally:
            del self.feed.push

    def _push_all(self, who, raw, flags, off, slot_of):
        for r in self.feed.push_all([self.slots[s] for s in who], raw, flags, offsets=off):
            self.log.append(log_entry(r))
            for i, sid in enumerate(r.ids):
                s = slot_of[int(sid)]
                rec = entry_record(r, i)
                self.calls[s].append(rec)
                self.status[s] = int(r.info[i]["status"])
                if rec["headers_ready"] and rec["link"] not in self.headers[s]:
                    self.headers[s][rec["link"]] = self.feed.headers(int(sid))


def check_against_model(run, blobs, cuts, end=True, model=M.Slot):
    """every call of every slot equals the model's, and so do the headers of every link that completed them"""
    for s, (b, c) in enumerate(zip(blobs, cuts)):
        slot, calls = M.run(b, c, end, slot=model())
        assert len(run.calls[s]) == len(calls), (s, len(run.calls[s]), len(calls))
        for k, (got, want) in enumerate(zip(run.calls[s], calls)):
            assert got == want, (s, k, {x: (got[x], want[x]) for x in got if got[x] != want[x] and x != "packets"},
                                 len(got["packets"]), len(want["packets"]))
        want_h = {k: l.headers[:3] for k, l in enumerate(slot.links) if len(l.headers) >= 3}
        assert run.headers[s] == want_h, (s, sorted(run.headers[s]), sorted(want_h))
        assert run.status[s] == 0
    return run


def joined(calls):
    """the packets of all calls, per link: {link: [(bytes, granulepos, eos, gap)]}"""
    out = {}
    for c in calls:
        if c["packets"]:
            out.setdefault(c["link"], []).extend(c["packets"])
    return out


def strict_packets(blob):
    """the audio packets of an undamaged single-link file by vbm_ogg_demux: [(bytes, granulepos, eos, 0)], headers"""
    sizes, hdr, body, offs, gp, eos = single(blob)
    pk = [(body[int(offs[k]):int(offs[k + 1])], int(gp[k]), int(eos[k]), 0) for k in range(len(gp))]
    return pk, [hdr[:sizes[0]], hdr[sizes[0]:sizes[0] + sizes[1]], hdr[sizes[0] + sizes[1]:]]
