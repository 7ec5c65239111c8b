"""Shared by test_ogg_chain_cpu.py and test_ogg_chain_gpu.py: chained corpora, the rule of csrc/ogg_chain.h as a page
walker in Python (the first yardstick; the second is vbm_ogg_demux on each link's bytes, ogg_demux_batch.single), and
the C calls of the split's host twin and device form over one interface."""
import functools
import struct

import numpy as np

from tests import ogg_demux_batch as B
from tests.ogg_demux_batch import ECAP, EINVAL, EOGG  # noqa: F401
from tests.ogg_pages import corruptions, parse, random_bytes, recrc, split_pages
from tests.ogg_twin import Result, Twin


# ---- the rule ----------------------------------------------------------------------------------------------------------

def walk(data, begin, end):
    """-> the link starts of the file data[begin:end]"""
    return [begin] + [p.pos for p in parse(data, begin, end) if p.flags & 2 and p.pos != begin]


def expected(blobs, first=0):
    """-> (file_links, link_offsets) of the batch B.pack(blobs, first) by the walker"""
    file_links, offs, at = [0], [], first
    for b in blobs:
        s = walk(b, 0, len(b))
        offs += [at + x for x in s]
        file_links.append(file_links[-1] + len(s))
        at += len(b)
    return np.array(file_links, np.int64), np.array(offs + [at], np.int64)


def links_of(blob):
    s = walk(blob, 0, len(blob)) + [len(blob)]
    return [blob[a:b] for a, b in zip(s[:-1], s[1:])]


# ---- corpora -----------------------------------------------------------------------------------------------------------

def reserial(blob, serialno):
    """the same pages under another serial number"""
    out = []
    for p in split_pages(blob):
        p[14:18] = struct.pack("<I", serialno)
        out.append(bytes(recrc(p)))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def small_links(n):
    """n short mono links of distinct serial numbers and lengths"""
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(40 + n)
    setup = v.Setup(1, 44100, 0.1)
    out = []
    for k in range(n):
        pk = [random_bytes(rng, int(x)) for x in rng.integers(0, 400, 1 + k % 5)]
        out.append(v.write_ogg(setup, pk, [(64 * (i + 1), i == len(pk) - 1) for i in range(len(pk))], serialno=1000 + k))
    return out


@functools.lru_cache(maxsize=None)
def class_links():
    """mono 8 kHz, stereo 44.1 kHz, 5.1 at 48 kHz: three sets of headers in one chain"""
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(41)
    out = []
    for k, (ch, rate, q) in enumerate([(1, 8000, 0.5), (2, 44100, 0.5), (6, 48000, 0.8)]):
        pk = [random_bytes(rng, n) for n in (17, 255, 900, 0, 4100)]
        out.append(v.write_ogg(v.Setup(ch, rate, q), pk, [(256 * (i + 1), i == 4) for i in range(5)], serialno=2000 + k))
    return out


def _with_empty_page(blob):
    """a 27-byte page (no segments) put in behind the first page, the later pages renumbered"""
    pages = split_pages(blob)
    empty = bytearray(pages[0][:27])
    empty[5], empty[26] = 0, 0
    pages.insert(1, empty)
    for k, p in enumerate(pages):
        p[18:22] = struct.pack("<I", k)
        recrc(p)
    return b"".join(bytes(p) for p in pages)


@functools.lru_cache(maxsize=None)
def shaped_links():
    """name -> link: the page shapes of the directed corpus, each under its own serial number"""
    d = dict(B.directed())
    out = {"headers alone": reserial(d["headers alone"], 3001),
           "unterminated": reserial(d["unterminated packet at the end"], 3002),
           "255 segments": reserial(d["packet over three pages"], 3003),
           "zero segments": _with_empty_page(small_links(3)[2]),
           "70 KB comment": reserial(d["header packet spans pages"], 3005)}
    assert any(p[26] == 255 for p in split_pages(out["255 segments"]))
    assert any(len(p) == 27 for p in split_pages(out["zero segments"]))
    assert B.single(out["zero segments"]) is not None
    return out


def _flag(blob, page, set_bits=0, clear_bits=0):
    pages = split_pages(blob)
    pages[page][5] = (pages[page][5] | set_bits) & ~clear_bits
    recrc(pages[page])
    return b"".join(bytes(p) for p in pages)


@functools.lru_cache(maxsize=None)
def chains():
    """name -> (file, the number of links the rule gives it, or None where only the walker says)"""
    a, b, c = small_links(3)
    sh = shaped_links()
    pa, pb = split_pages(a), split_pages(b)
    j = b"".join
    out = {"1 link": (a, 1), "2 links": (a + b, 2), "3 links": (a + b + c, 3), "65 links": (j(small_links(65)), 65),
           "three classes": (j(class_links()), 3),
           "headers alone in the middle": (a + sh["headers alone"] + b, 3),
           "headers alone at the end": (a + sh["headers alone"], 2),
           "unterminated packet, then a link": (sh["unterminated"] + b, 2),
           "255 segments": (a + sh["255 segments"] + b, 3),
           "zero segments": (a + sh["zero segments"] + b, 3),
           "70 KB comment in the middle": (a + sh["70 KB comment"] + b, 3),
           "first page without the flag": (_flag(a, 0, clear_bits=2) + b, 2),
           "flag on a later page": (_flag(c, 2, set_bits=2), 2),
           "multiplexed start": (j(bytes(p) for p in pa[:1] + pb[:1] + pa[1:] + pb[1:]), 2)}
    return out


# The middle link of three under every corruptions variant: which links the rule finds, and which of them the demux then
# accepts.  A page that no longer parses ends the walk, so everything behind it stays with the link it lies in; a page
# that still parses (bad CRC, serial, sequence, continuation) costs its own link only.
MIDDLE = {"capture pattern": [False],                        # the link's first page: it never starts, link 0 takes it all
          "capture pattern of page 2": [True, False],
          "version": [True, False],
          "crc": [True, False, True],
          "truncated page": [True, False],                   # the page takes a byte of the next link, which then does not parse
          # 20 bytes of a first page, completed by 7 of the next link's: a page of no segments that carries the flag
          "truncated header": [True, True, False],
          "second serial": [True, False, True],
          "out of sequence": [True, False, True],
          "continuation without the flag": [True, False, True],
          "fewer than three packets": [True, False, True],
          "empty": [True, True]}


@functools.lru_cache(maxsize=None)
def middle_corruptions():
    """name -> file of three links whose middle one is corrupted"""
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(43)
    # the middle link needs a page that continues a packet
    pk = [random_bytes(rng, n) for n in (300, 70000, 20, 700)]
    mid = v.write_ogg(v.Setup(1, 44100, 0.1), pk, [(128 * (i + 1), i == 3) for i in range(4)], serialno=4000)
    a, b, _ = small_links(3)
    return {name: a + bad + b for name, bad in corruptions(mid).items()}


def alignment_batch():
    """chains with one to three bytes of filler between them: with the batch's first byte at 0 to 7, starts at every
    alignment"""
    a, b, c = small_links(3)
    sh = shaped_links()
    blobs = []
    for k, x in enumerate([a + b, sh["255 segments"] + c, b, c + sh["zero segments"] + a, sh["70 KB comment"], a + c]):
        blobs += [b"\xee" * (1 + k % 3), x]
    return blobs


def many_files():
    """1025 files, more than one step of the block scan, most of them empty"""
    a, b, c = small_links(3)
    blobs = [b""] * 1025
    blobs[3], blobs[700], blobs[1023], blobs[1024] = a + b, c, a + b + c, b + a
    return blobs


@functools.lru_cache(maxsize=None)
def two_link_file():
    blob, _ = B.six_packet_file()
    return blob, reserial(blob, 5001)


# ---- the host twin and the device calls (ogg_twin.Twin) ------------------------------------------------------------------

class Chain(Twin):
    """A splitter and its buffers"""

    def __init__(self, impl, max_files, max_bytes):
        super().__init__(impl, "chain", max_files, max_bytes)

    def split_raw(self, nfiles, data_ptr, off_ptr, file_links_ptr, link_offsets_ptr, link_cap):
        return self.call("chain_split", nfiles, data_ptr, off_ptr, file_links_ptr, link_offsets_ptr, link_cap)

    def split(self, data, offsets, link_cap, canary=8):
        """data: uint8 numpy or an address -> Result: .file_links [n + 1], .link_offsets [link_cap + 1], .status,
        .touched (link_offsets differs from its blank pattern), .canaries_ok (`canary` entries behind each output)"""
        n = len(offsets) - 1
        if isinstance(data, np.ndarray):
            data = self.upload(data)
        fl, lo = self.guarded(n + 1, np.int64, canary), self.guarded(link_cap + 1, np.int64, canary)
        off = np.ascontiguousarray(offsets, np.int64)
        rc = self.split_raw(n, data, off.ctypes.data, self.ptr(fl), self.ptr(lo), link_cap)
        assert rc == 0, (rc, self.lib.vbm_last_error())
        r = Result()
        r.status = self.status()
        (r.file_links, _, ok0), (r.link_offsets, r.touched, ok1) = self.unguard(fl, n + 1), self.unguard(lo, link_cap + 1)
        r.canaries_ok = ok0 and ok1
        return r


def run(impl, blobs, first=0, slack=0):
    """the split of one batch whose first file starts at byte `first`, with room for exactly the links the rule gives it
    (+ slack) -> (file_links, link_offsets [total + 1])"""
    data, offsets = B.pack(blobs, first)
    want_fl, _ = expected(blobs, first)
    total = int(want_fl[-1])
    c = Chain(impl, max(1, len(blobs)), int(offsets[-1] - offsets[0]))
    try:
        r = c.split(data, offsets, total + slack)
        assert r.status == 0 and r.canaries_ok, r.status
        return r.file_links, r.link_offsets[:total + 1]
    finally:
        c.close()


def check_split(impl, blobs, first=0):
    """the split equals the walker's -> the links as bytes"""
    fl, lo = run(impl, blobs, first)
    want_fl, want_lo = expected(blobs, first)
    assert np.array_equal(fl, want_fl), (fl, want_fl)
    assert np.array_equal(lo, want_lo), (lo, want_lo)
    raw = b"".join(blobs)
    return [raw[int(a) - first:int(b) - first] for a, b in zip(lo[:-1], lo[1:])]


def check_demux(impl, blobs, first=0):
    """... and the batch demux over the link offsets gives every link what vbm_ogg_demux gives its bytes alone ->
    [link accepted]"""
    links = check_split(impl, blobs, first)
    _, lo = expected(blobs, first)
    data, _ = B.pack(blobs, first)
    b = B.Batch(impl, max(1, len(links)), len(data) - first)
    try:
        info, totals = b.scan(data, lo)
        res = b.fill(totals)
    finally:
        b.close()
    assert res.status == 0 and res.canaries_ok
    B.check_csr(info, totals, res)
    ok = []
    for k, link in enumerate(links):
        want = B.single(link)
        assert B.same(B.file_view(info, res, k), want), k
        ok.append(want is not None)
    return ok
