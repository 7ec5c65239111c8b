"""Shared by test_ogg_feed_cpu.py and test_ogg_feed_gpu.py: the C calls of the incremental Ogg demux (vbm_ogg_feed_*) over
one interface for the host twin and the device, and the scenarios both files run.  A scenario drives a Feed through a
fixed list of calls, asserts what the issue's rules say against the single-file yardstick (vbm_ogg_demux), and returns
the log of every call's info structs, totals and outputs, so that the device's log can be compared with the twin's."""
import ctypes as C
import functools

import numpy as np

from tests.ogg_demux_batch import ECAP, EINVAL, EOGG, directed, mixed, same, single, six_packet_file
from tests.ogg_pages import pack, split_pages
from tests.ogg_twin import Result, Twin, lib as _lib  # noqa: F401

EBIG = -1003
BIG = 1 << 17                     # packet / header capacity that holds every packet of the corpora
CHUNKS = (26, 27, 28, 255, 256, 4096)


def _info_dtype():
    from vorbis_aotuv_lancer_amd.stream import FEED_INFO
    return FEED_INFO


class Feed(Twin):
    """A feed and its buffers.  Every call is appended to .log."""

    def __init__(self, impl, max_streams, max_call_bytes, carry=65307, packet=BIG, header=BIG):
        super().__init__(impl, "feed", max_streams, max_call_bytes, carry, packet, header)
        self.log = []

    def scan_raw(self, n, ids_ptr, data_ptr, off_ptr, end_ptr, info_ptr, totals_ptr):
        return self.call("feed_scan", n, ids_ptr, data_ptr, off_ptr, end_ptr, info_ptr, totals_ptr)

    def fill_raw(self, pay, pcap, offs, gp, eos, kcap):
        return self.call("feed_fill", pay, pcap, offs, gp, eos, kcap)

    def scan(self, ids, chunks, end=None, first=0):
        """chunks back to back behind `first` bytes of 0xEE -> (info, totals) as numpy"""
        n = len(ids)
        ids = np.ascontiguousarray(ids, np.int32)
        raw, off = pack(chunks, first)
        flags = None if end is None else np.ascontiguousarray(np.broadcast_to(np.asarray(end, np.uint8), (n,)))
        meta = self.new(16 + n * _info_dtype().itemsize, np.uint8)
        rc = self.scan_raw(n, ids.ctypes.data, self.upload(raw), off.ctypes.data,
                           None if flags is None else flags.ctypes.data, self.ptr(meta) + 16, self.ptr(meta))
        assert rc == 0, (rc, self.lib.vbm_last_error())
        meta = self.back(meta)
        info, totals = meta[16:].view(_info_dtype()).copy(), meta[:16].view(np.int64).copy()
        self.log.append(("scan", info.tobytes(), totals.tolist()))
        return info, totals

    def fill(self, totals, short=None, canary=8):
        """buffers of exactly the totals' sizes (short: 'packets' / 'payload' tells fill one less), `canary` elements of
        blank bytes behind each -> Result of numpy arrays without the canaries, .status, .touched, .canaries_ok"""
        P, B = (int(x) for x in totals)
        # one buffer of blank bytes for all four outputs (one fill, one copy back): offsets, granulepos, payload, eos
        sizes = {"offsets": (P + 1, 8), "granulepos": (P, 8), "payload": (B, 1), "eos": (P, 1)}
        at, where = 0, {}
        for name, (n, w) in sizes.items():
            where[name] = at
            at += (n + canary) * w
        buf = self.guarded(at, np.uint8, 0)
        ptr = {name: self.ptr(buf) + where[name] for name in sizes}
        caps = {"packets": P, "payload": B}
        if short:
            caps[short] -= 1
        rc = self.fill_raw(ptr["payload"], caps["payload"], ptr["offsets"], ptr["granulepos"], ptr["eos"], caps["packets"])
        assert rc == 0, (rc, self.lib.vbm_last_error())
        r = Result()
        r.status = self.status()
        r.touched, r.canaries_ok = False, True
        back = self.back(buf)
        for name, (n, w) in sizes.items():
            a, touched, ok = self.unguard(back[where[name]:where[name] + (n + canary) * w], n * w)
            r.touched, r.canaries_ok = r.touched or touched, r.canaries_ok and ok
            setattr(r, name, a.view(np.int64 if w == 8 else np.uint8).copy())
        self.log.append(("fill", r.status, r.touched, r.canaries_ok, r.payload.tobytes(), r.offsets.tolist(),
                         r.granulepos.tolist(), r.eos.tolist()))
        return r

    def push(self, ids, chunks, end=None, first=0):
        info, totals = self.scan(ids, chunks, end, first)
        res = self.fill(totals)
        assert res.status == 0 and res.canaries_ok
        check_csr(info, totals, res)
        return info, totals, res

    def headers(self, slot):
        """-> (sizes [3], bytes) or None while they are not ready"""
        sizes = (C.c_int * 3)()
        if self.lib.vbm_ogg_feed_headers(self.h, slot, None, 0, sizes, self.q()) != 0:
            return None
        n = sum(sizes)
        buf = np.zeros(n + 8, np.uint8)
        assert self.lib.vbm_ogg_feed_headers(self.h, slot, buf.ctypes.data, n, sizes, self.q()) == 0
        assert not buf[n:].any()
        self.log.append(("headers", slot, list(sizes), buf[:n].tobytes()))
        return list(sizes), buf[:n].tobytes()

    def reset(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        assert self.lib.vbm_ogg_feed_reset_streams(self.h, len(ids), ids.ctypes.data, self.q()) == 0


def check_csr(info, totals, res):
    P, B = (int(x) for x in totals)
    assert res.offsets[0] == 0 and res.offsets[P] == B and (np.diff(res.offsets) >= 0).all()
    pk, nb = info["packets"], info["payload_bytes"]
    assert (pk >= 0).all() and (nb >= 0).all()
    assert np.array_equal(info["packet_base"], np.cumsum(pk) - pk) and np.array_equal(info["payload_base"], np.cumsum(nb) - nb)
    assert (int(pk.sum()), int(nb.sum())) == (P, B)
    assert np.array_equal(res.offsets[info["packet_base"]], info["payload_base"])
    assert np.array_equal(res.offsets[info["packet_base"] + pk], info["payload_base"] + nb)


class Streams:
    """the concatenation of the calls' outputs, slot by slot"""

    def __init__(self):
        self.acc = {}
        self.status = {}
        self.info = {}

    def add(self, ids, info, res):
        ids = [int(x) for x in ids]
        self.status.update(zip(ids, info["status"].tolist()))
        for i, slot in enumerate(ids):
            self.info[slot] = info[i]
            if slot not in self.acc:
                self.acc[slot] = dict(payload=bytearray(), offsets=[0], gp=[], eos=[])
        for i in np.flatnonzero(info["packets"]).tolist():
            slot, fi = ids[i], info[i]
            a = self.acc[slot]
            p, n, at, nb = int(fi["packet_base"]), int(fi["packets"]), int(fi["payload_base"]), int(fi["payload_bytes"])
            a["offsets"] += (res.offsets[p + 1:p + n + 1] - at + len(a["payload"])).tolist()
            a["payload"] += res.payload[at:at + nb].tobytes()
            a["gp"] += res.granulepos[p:p + n].tolist()
            a["eos"] += res.eos[p:p + n].tolist()

    def packets(self, slot):
        """what was delivered for the slot, without the headers"""
        a = self.acc[slot]
        return bytes(a["payload"]), list(a["offsets"]), list(a["gp"]), list(a["eos"])

    def view(self, feed, slot):
        """-> what single() returns for a file, or None while the headers are not complete"""
        h = feed.headers(slot)
        if h is None:
            return None
        a = self.acc[slot]
        return (h[0], h[1], bytes(a["payload"]), np.array(a["offsets"], np.int64), np.array(a["gp"], np.int64),
                np.array(a["eos"], np.uint8))


def calls_of(blobs, cs, slots=None):
    """every blob in its own slot, `cs` bytes per call, `end` on each blob's last chunk -> [(ids, chunks, end)]"""
    slots = list(range(len(blobs))) if slots is None else slots
    out, pos = [], 0
    longest = max(len(b) for b in blobs)
    while pos < longest or not out:
        ids, chunks, end = [], [], []
        for s, b in zip(slots, blobs):
            if pos < len(b) or pos == 0:
                ids.append(s)
                chunks.append(b[pos:pos + cs])
                end.append(pos + cs >= len(b))
        out.append((ids, chunks, end))
        pos += cs
    return out


def feed_all(feed, blobs, cs, streams=None, slots=None, tail_calls=0):
    """calls_of through feed.push; tail_calls: calls with 40 more bytes for every slot after the last.  -> Streams"""
    streams = streams or Streams()
    slots = list(range(len(blobs))) if slots is None else slots
    for ids, chunks, end in calls_of(blobs, cs, slots):
        info, totals, res = feed.push(ids, chunks, end)
        streams.add(ids, info, res)
    for _ in range(tail_calls):
        before = dict(streams.status)
        info, totals, res = feed.push(slots, [b"OggS" + bytes(36)] * len(slots))
        assert totals.tolist() == [0, 0]
        streams.add(slots, info, res)
        assert streams.status == before
    return streams


@functools.lru_cache(maxsize=None)
def corpus():
    """(name, blob, single(blob)) of directed(), mixed(), a bare capture pattern and random bytes"""
    rng = np.random.default_rng(77)
    out = list(directed()) + list(mixed()) + [("bare capture pattern", b"OggS"),
                                              ("random bytes", rng.integers(0, 256, 5000, dtype=np.uint8).tobytes())]
    return [(name, blob, single(blob)) for name, blob in out]


# ---- scenarios: impl -> log ------------------------------------------------------------------------------------------------

def scenario_corpus(impl, cs):
    """items 1, 3 and 4: every file of the corpus in its own slot of the same calls, cs bytes per call (None: whole).  A
    good file's concatenation equals single(); a rejected one ends as VBM_EOGG and what it delivered does not depend on
    cs (the caller compares the returned deliveries across chunk sizes); bytes after the end change nothing."""
    files = corpus()
    blobs = [b for _, b, _ in files]
    step = cs or max(len(b) for b in blobs)
    feed = Feed(impl, len(blobs), step * len(blobs) + 64 * len(blobs))
    try:
        st = feed_all(feed, blobs, step, tail_calls=1)
        delivered = {}
        for slot, (name, blob, want) in enumerate(files):
            if want is None:
                assert st.status[slot] == EOGG, (name, cs, st.status[slot])
            else:
                assert st.status[slot] == 0, (name, cs, st.status[slot])
                assert same(st.view(feed, slot), want), (name, cs)
            delivered[name] = (st.status[slot], st.packets(slot))
        name = "unterminated packet at the end"
        slot = [n for n, _, _ in files].index(name)
        assert st.status[slot] == 0 and len(st.packets(slot)[2]) == 240         # the 240 small packets, not the open one
        return feed.log, delivered
    finally:
        feed.close()


def _cuts_scenario(impl, blob, bounds, cuts, check_first):
    """slot k gets blob cut at cuts[k] (a sorted tuple of positions), one piece per call, `end` with the last"""
    n = len(cuts)
    ncalls = len(cuts[0]) + 1
    feed = Feed(impl, n, sum(max(b - a for a, b in zip((0,) + c, c + (len(blob),))) for c in cuts), carry=8192)
    want = single(blob)
    upto_bound = {b: single(blob[:b]) for b in set(bounds) | {0}}
    try:
        st = Streams()
        ids = list(range(n))
        for j in range(ncalls):
            chunks = [blob[((0,) + c)[j]:(c + (len(blob),))[j]] for c in cuts]
            info, totals, res = feed.push(ids, chunks, end=(j == ncalls - 1))
            st.add(ids, info, res)
            if j == 0 and check_first:
                for k in ids:
                    cut = cuts[k][0]
                    assert info[k]["pending"] + info[k]["consumed"] == cut, k
                    whole = max([b for b in bounds if b <= cut], default=0)
                    assert info[k]["consumed"] == whole, k
                    upto = upto_bound[whole]
                    got = st.packets(k)
                    if upto is None:                            # fewer than three packets on the whole pages
                        assert got == (b"", [0], [], []), k
                    else:
                        assert (got[0], got[1], got[2], got[3]) == (upto[2], upto[3].tolist(), upto[4].tolist(),
                                                                    upto[5].tolist()), k
        for k in ids:
            assert st.status[k] == 0 and same(st.view(feed, k), want), k
        return feed.log
    finally:
        feed.close()


def scenario_every_cut(impl):
    blob, bounds = six_packet_file()
    return _cuts_scenario(impl, blob, bounds, [(k,) for k in range(len(blob) + 1)], True)


def scenario_random_cuts(impl):
    blob, bounds = six_packet_file()
    rng = np.random.default_rng(31)
    cuts = [tuple(sorted(int(x) for x in rng.integers(0, len(blob) + 1, 2))) for _ in range(len(blob) + 1)]
    return _cuts_scenario(impl, blob, bounds, cuts, False)


def scenario_byte_by_byte(impl):
    """one byte per call for the first 600 bytes, four slots in phase, then the rest at once"""
    blob, _ = six_packet_file()
    feed = Feed(impl, 4, 4 * len(blob))
    try:
        st, ids = Streams(), [0, 1, 2, 3]
        for k in range(600):
            info, totals, res = feed.push(ids, [blob[k:k + 1]] * 4)
            st.add(ids, info, res)
        info, totals, res = feed.push(ids, [blob[600:]] * 4, end=True)
        st.add(ids, info, res)
        want = single(blob)
        for k in ids:
            assert st.status[k] == 0 and same(st.view(feed, k), want), k
        return feed.log
    finally:
        feed.close()


def scenario_alignment(impl, first):
    """chunks that start at every alignment in the call's data (`first` bytes of garbage in front, one to three between
    the chunks, given to slots of their own) and leave page tails of every length mod 4"""
    blob, _ = six_packet_file()
    feed = Feed(impl, 8, 8 * len(blob))
    try:
        st, ids, one, two, end = Streams(), [], [], [], []
        pos = 0
        for j in range(4):
            cut = len(blob) - 1500 + j                          # inside the last page
            ids += [4 + j, j]
            gap = (j - pos) % 4 or 4                            # chunk j starts at first + j (mod 4)
            one += [b"\xee" * gap, blob[:cut]]
            pos += gap + cut
            two += [b"\xee" * (1 + (j + 1) % 3), blob[cut:]]
            end += [0, 1]
        info, totals, res = feed.push(ids, one, first=first)
        st.add(ids, info, res)
        assert sorted(int(x) % 4 for x in info["pending"][1::2]) == [0, 1, 2, 3]
        assert sorted((first + int(x)) % 4 for x in np.cumsum([len(c) for c in one])[0::2]) == [0, 1, 2, 3]
        info, totals, res = feed.push(ids, two, end, first=(first + 1) % 4)
        st.add(ids, info, res)
        for k in range(4):
            assert st.status[k] == 0 and same(st.view(feed, k), single(blob)), k
            assert st.status[4 + k] == 0 and st.info[4 + k]["pending"] == len(one[2 * k]) + len(two[2 * k])
        return feed.log
    finally:
        feed.close()


def scenario_too_big(impl, which):
    """item 5: the slot in the middle exceeds one capacity; its neighbours hold a good file in the same calls"""
    good, _ = six_packet_file()
    d = dict(directed())
    if which == "packet":
        bad, caps, cs = d["packet over three pages"], dict(packet=65536), 4096
    elif which == "header":
        bad, caps, cs = d["header packet spans pages"], dict(header=65536), 4096
    else:                                                       # a page of 255 segments cut in its middle
        bad, caps = d["packet over three pages"], dict(carry=4096)
        pages = split_pages(bad)
        big = next(i for i, p in enumerate(pages) if p[26] == 255)
        cs = sum(len(p) for p in pages[:big]) + len(pages[big]) // 2
    feed = Feed(impl, 3, 3 * max(cs, len(good)), **caps)
    alone = Feed(impl, 3, 3 * max(cs, len(good)), **caps)
    try:
        st = feed_all(feed, [good, bad, good], cs)
        ref = feed_all(alone, [good, good], cs, slots=[0, 2])
        assert st.status == {0: 0, 1: EBIG, 2: 0}, st.status
        for k in (0, 2):
            assert st.packets(k) == ref.packets(k) and same(st.view(feed, k), single(good))
        if which != "header":                                   # the 240 packets in front of the big one were delivered
            assert len(st.packets(1)[2]) == 240
        # sticky: more bytes change nothing
        info, totals, res = feed.push([1], [bad[:100]])
        assert info[0]["status"] == EBIG and totals.tolist() == [0, 0]
        return feed.log
    finally:
        feed.close()
        alone.close()


def scenario_capacity_short(impl, short):
    """item 6: a fill one short writes nothing and leaves the state alone: filled again with room, and fed on, the
    stream comes out as from a feed that never fell short"""
    blob = dict(mixed())["small_packets"]
    cuts = (0, 20000, 50000, len(blob))
    feeds = [Feed(impl, 2, 2 * len(blob)), Feed(impl, 2, 2 * len(blob))]
    try:
        sts = [Streams(), Streams()]
        for j in range(3):
            chunks = [blob[cuts[j]:cuts[j + 1]]] * 2
            for f, (feed, st) in enumerate(zip(feeds, sts)):
                info, totals = feed.scan([0, 1], chunks, end=(j == 2))
                if f == 0 and j == 1:
                    assert totals[0] > 0 and totals[1] > 0
                    res = feed.fill(totals, short=short)
                    assert res.status == ECAP and not res.touched and res.canaries_ok
                res = feed.fill(totals)
                assert res.status == 0 and res.canaries_ok
                st.add([0, 1], info, res)
        for k in (0, 1):
            assert sts[0].packets(k) == sts[1].packets(k)
            assert same(sts[0].view(feeds[0], k), single(blob)) and same(sts[1].view(feeds[1], k), single(blob))
        # a scan that is committed is not filled twice
        res = feeds[0].fill([0, 0])
        assert res.status == EINVAL and not res.touched
        return feeds[0].log
    finally:
        for f in feeds:
            f.close()


def scenario_slots(impl):
    """item 7: reset, unlisted slots, zero-length chunks"""
    blob, _ = six_packet_file()
    other = mixed()[1][1]                                       # a good file with another serial number
    assert single(other) is not None
    feed = Feed(impl, 3, 3 * max(len(blob), len(other)))
    try:
        st = Streams()
        info, totals, res = feed.push([0, 2], [blob[:700], blob[:900]])
        st.add([0, 2], info, res)
        pend = int(info[1]["pending"])
        # slot 2 is not listed, slot 0 gets nothing: both keep their carry
        info, totals, res = feed.push([0, 1], [b"", blob])
        st.add([0, 1], info, res)
        assert info[0]["packets"] == 0 and info[0]["consumed"] == 0 and info[0]["status"] == 0
        info, totals, res = feed.push([2, 0], [blob[900:], blob[700:]], end=True)
        st.add([2, 0], info, res)
        assert pend > 0 and info[0]["consumed"] > pend
        info, totals, res = feed.push([1], [b""], end=True)
        st.add([1], info, res)
        for k in range(3):
            assert st.status[k] == 0 and same(st.view(feed, k), single(blob)), k
        # an ended slot takes nothing more; after a reset it takes a second file with another serial number
        info, totals, res = feed.push([1], [other[:5000]])
        assert totals.tolist() == [0, 0] and info[0]["consumed"] == 0
        feed.reset([1])
        assert feed.headers(1) is None
        st2 = feed_all(feed, [other], 50000, slots=[1])
        assert st2.status[1] == 0 and same(st2.view(feed, 1), single(other))
        assert st2.info[1]["serialno"] != st.info[1]["serialno"]
        assert same(st.view(feed, 0), single(blob))            # its neighbours' headers are where they were
        return feed.log
    finally:
        feed.close()


def check_einval(impl):
    """item 7: every VBM_EINVAL, and that a refused call leaves the feed usable"""
    blob, _ = six_packet_file()
    feed = Feed(impl, 4, 20000)
    try:
        i32 = lambda *a: np.array(a, np.int32)                  # noqa: E731
        i64 = lambda *a: np.array(a, np.int64)                  # noqa: E731
        data = feed.new(2000, np.uint8)
        meta = feed.new(16 + 4 * _info_dtype().itemsize, np.uint8)
        d, info, totals = feed.ptr(data), feed.ptr(meta) + 16, feed.ptr(meta)

        def scan(ids, off, data=d, info=info, totals=totals, n=None):
            return feed.scan_raw(len(ids) if n is None else n, ids.ctypes.data, data, off.ctypes.data, None, info, totals)

        assert feed.fill_raw(None, 0, feed.ptr(feed.new(1, np.int64)), None, None, 0) == EINVAL   # fill without a scan
        assert scan(i32(1, 1), i64(0, 10, 20)) == EINVAL        # listed twice
        assert scan(i32(0, 4), i64(0, 10, 20)) == EINVAL        # out of range
        assert scan(i32(0, -1), i64(0, 10, 20)) == EINVAL
        assert scan(i32(0, 1), i64(0, 20, 10)) == EINVAL        # offsets decrease
        assert scan(i32(0, 1), i64(-1, 0, 10)) == EINVAL
        assert scan(i32(0, 1), i64(0, 500, 20001)) == EINVAL     # above max_call_bytes
        assert scan(i32(0, 1, 2, 3, 0), i64(0, 0, 0, 0, 0, 0)) == EINVAL      # n above max_streams
        assert scan(i32(0), i64(0), n=-1) == EINVAL
        assert scan(i32(0, 1), i64(0, 10, 20), data=None) == EINVAL
        assert scan(i32(0, 1), i64(0, 10, 20), info=None) == EINVAL
        assert scan(i32(0, 1), i64(0, 10, 20), totals=None) == EINVAL
        assert feed.scan_raw(2, None, d, i64(0, 10, 20).ctypes.data, None, info, totals) == EINVAL
        assert feed.scan_raw(2, i32(0, 1).ctypes.data, d, None, None, info, totals) == EINVAL
        assert feed.lib.vbm_ogg_feed_reset_streams(feed.h, 2, i32(2, 2).ctypes.data, feed.q()) == EINVAL
        assert feed.lib.vbm_ogg_feed_reset_streams(feed.h, 1, i32(9).ctypes.data, feed.q()) == EINVAL
        sizes = (C.c_int * 3)()
        assert feed.lib.vbm_ogg_feed_headers(feed.h, 0, None, 0, sizes, feed.q()) == EINVAL        # not ready
        assert feed.lib.vbm_ogg_feed_headers(feed.h, 4, None, 0, sizes, feed.q()) == EINVAL
        # the other kind of feed
        wrong = feed.lib.vbm_ogg_feed_scan if impl == "host" else feed.lib.vbm_host_ogg_feed_scan
        args = (feed.h, 1, i32(0).ctypes.data, d, i64(0, 10).ctypes.data, None, info, totals)
        assert wrong(*args, None) == EINVAL if impl == "host" else wrong(*args) == EINVAL
        # nothing was enqueued or changed: the feed works, and the ids of a refused call are not remembered
        info_, totals_ = feed.scan([1, 0], [blob[:500], blob[:400]])
        out = feed.new(8, np.int64)
        assert feed.fill_raw(None, -1, feed.ptr(out), None, None, 0) == EINVAL
        assert feed.fill_raw(None, 0, None, None, None, 0) == EINVAL
        assert feed.fill_raw(None, 1, feed.ptr(out), None, None, 0) == EINVAL
        assert feed.fill_raw(None, 0, feed.ptr(out), None, None, 1) == EINVAL
        res = feed.fill(totals_)
        assert res.status == 0
        st = Streams()
        st.add([1, 0], info_, res)
        info_, totals_, res = feed.push([0, 1], [blob[400:], blob[500:]], end=True)
        st.add([0, 1], info_, res)
        assert same(st.view(feed, 0), single(blob)) and same(st.view(feed, 1), single(blob))
        sz, _ = feed.headers(0)
        assert feed.lib.vbm_ogg_feed_headers(feed.h, 0, np.zeros(sum(sz), np.uint8).ctypes.data, sum(sz) - 1, sizes,
                                             feed.q()) == EINVAL
    finally:
        feed.close()
    for bad in ((0, 10, 1, 1, 1), (1, -1, 1, 1, 1), (1, 10, 0, 1, 1), (1, 10, 65308, 1, 1), (1, 10, 1, 0, 1), (1, 10, 1, 1, 0)):
        h = C.c_void_p()
        assert feed.fn("feed_create")(C.byref(h), *bad) == EINVAL, bad
