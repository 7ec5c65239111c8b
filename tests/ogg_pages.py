"""Ogg pages for the tests, and the rules over them, each stated once: the page-parse test of csrc/ogg_chain.h (parse, and
the walkers that are loops over it), the group rule of csrc/ogg_select.h (group_step), the page checksum in two forms of
the tests' own, page builders, and the helpers the corpora share.  Plain Python and numpy; nothing here is taken from
the product."""
import collections
import ctypes as C
import functools
import mmap
import struct

import numpy as np

MARK = b"\x01vorbis"


# ---- the checksum ------------------------------------------------------------------------------------------------------

def _table():
    t = []
    for i in range(256):
        r = i << 24
        for _ in range(8):
            r = ((r << 1) ^ 0x04c11db7) & 0xffffffff if r & 0x80000000 else (r << 1) & 0xffffffff
        t.append(r)
    return t


_T = _table()


@functools.lru_cache(maxsize=4096)
def page_crc(page):
    """the checksum of a page, its own field counted as zero"""
    r = 0
    for i, b in enumerate(page):
        if 22 <= i < 26:
            b = 0
        r = ((r << 8) & 0xffffffff) ^ _T[(r >> 24) ^ b]
    return r


def crc_bitwise(data):
    """doc/framing.html:363-366: direct CRC-32, polynomial 0x04c11db7, initial value and final XOR 0"""
    r = 0
    for byte in data:
        r ^= byte << 24
        for _ in range(8):
            r = ((r << 1) ^ 0x04c11db7) & 0xffffffff if r & 0x80000000 else (r << 1) & 0xffffffff
    return r


def recrc(page):
    """a bytearray page with its checksum field set anew -> the same bytearray"""
    page[22:26] = struct.pack("<I", page_crc(bytes(page)))
    return page


# ---- the parse rule, and the walkers over it ---------------------------------------------------------------------------

Page = collections.namedtuple("Page", "pos size flags serial seq granule crc nseg body")    # body: where the body starts


def parse(data, begin, end):
    """The pages of data[begin:end] by the parse test of csrc/ogg_chain.h: 27 bytes with the capture pattern and version
    0, a lacing table that fits, a body that fits.  Stops at the first position that fails it."""
    pos = begin
    while end - pos >= 27:
        h = data[pos:pos + 27]
        if h[:4] != b"OggS" or h[4] != 0:
            break
        nseg = h[26]
        if end - pos - 27 < nseg:
            break
        body = sum(data[pos + 27:pos + 27 + nseg])
        if end - pos - 27 - nseg < body:
            break
        flags, granule, serial, seq, crc = struct.unpack_from("<BqIII", h, 5)
        yield Page(pos, 27 + nseg + body, flags, serial, seq, granule, crc, nseg, pos + 27 + nseg)
        pos += 27 + nseg + body


def body7(data, p):
    """the first 7 bytes of the body of page p of data, fewer if it has fewer: what group_step looks at"""
    return data[p.body:min(p.body + 7, p.pos + p.size)]


def split_pages(blob, as_bytes=False):
    """the pages of a file that parses to its end -> [bytearray] for callers that edit them, or [bytes]"""
    out = [blob[p.pos:p.pos + p.size] for p in parse(blob, 0, len(blob))]
    assert sum(len(p) for p in out) == len(blob), "not whole pages"
    return [bytes(p) for p in out] if as_bytes else [bytearray(p) for p in out]


@functools.lru_cache(maxsize=4096)
def _checked_page(page):
    p = next(parse(page, 0, len(page)))
    assert crc_bitwise(page[:22] + b"\0\0\0\0" + page[26:]) == p.crc, "page CRC"
    return {"flags": p.flags, "granule": p.granule, "serial": p.serial, "seq": p.seq, "lacing": list(page[27:27 + p.nseg]),
            "body": page[27 + p.nseg:]}


def parse_pages(blob):
    """the pages of a file that parses to its end, as dicts, the checksum of each checked bitwise (a page seen before is
    taken from a cache)"""
    blob = bytes(blob)
    out, at = [], 0
    for p in parse(blob, 0, len(blob)):
        out.append(_checked_page(blob[p.pos:p.pos + p.size]))
        at = p.pos + p.size
    assert at == len(blob), f"no page at byte {at}"
    return out


def packets_of(pages):
    """parse_pages' dicts -> the packets, by the lacing values"""
    out, cur, open_ = [], b"", False
    for pg in pages:
        assert bool(pg["flags"] & 1) == open_, "continued-packet flag"
        at = 0
        for lv in pg["lacing"]:
            cur += pg["body"][at:at + lv]
            at += lv
            if lv < 255:
                out.append(cur)
                cur = b""
        open_ = bool(pg["lacing"]) and pg["lacing"][-1] == 255
    assert not open_
    return out


# ---- the group rule ----------------------------------------------------------------------------------------------------

GROUP_START = (True, False, 0)


def group_step(state, head, s, body7):
    """The group rule of csrc/ogg_select.h for one page.  state: (in_heads, chosen, serial); head: the page starts a
    stream (or is the first there is); s: its serial number; body7: the first 7 bytes of its body, fewer if it has
    fewer.  -> (the state behind the page, whether the page is the one that chose a stream).  The page is kept when
    the new state has chosen and serial == s."""
    in_heads, chosen, serial = state
    if head and not in_heads:
        in_heads, chosen = True, False
    if not head:
        in_heads = False
    picked = head and not chosen and body7 == MARK
    if picked:
        chosen, serial = True, s
    return (in_heads, chosen, serial), picked


# ---- page builders -----------------------------------------------------------------------------------------------------

def page(serial, seq, lacing, body, flags=0, granule=0):
    assert len(lacing) <= 255 and sum(lacing) == len(body)
    p = bytearray(b"OggS\0" + bytes([flags]) + struct.pack("<qIII", granule, serial, seq, 0) + bytes([len(lacing)])
                  + bytes(lacing) + body)
    return bytes(recrc(p))


def lay(packets, serial, max_segs=255, bos=True, eos=True, first_alone=True):
    """packets -> the pages of one logical stream: at most max_segs segments per page, the first packet on a page of
    its own, continuation flags where a page begins inside a packet"""
    segs = []                                             # (the segment's bytes, it ends its packet, the packet)
    for k, pk in enumerate(packets):
        n = len(pk) // 255 + 1
        for i in range(n):
            segs.append((pk[255 * i:255 * i + 255], i == n - 1, k))
    pages, at, seq, open_packet, done = [], 0, 0, False, 0
    while at < len(segs):
        take = max_segs
        if first_alone and seq == 0:
            take = min(take, len(packets[0]) // 255 + 1)
        part = segs[at:at + take]
        at += len(part)
        flags = (1 if open_packet else 0) | (2 if bos and seq == 0 else 0) | (4 if eos and at == len(segs) else 0)
        ends = sum(1 for s in part if s[1])
        done += ends
        pages.append(page(serial, seq, [len(s[0]) for s in part], b"".join(s[0] for s in part), flags,
                          64 * done if ends else -1))
        open_packet = not part[-1][1]
        seq += 1
    return pages


def interleave(streams, seed):
    """page lists of one group -> one page list: every stream's first page first, in the order given, then the rest
    merged in a seeded order that keeps each stream's own"""
    rng = np.random.default_rng(seed)
    out = [s[0] for s in streams]
    rest = [list(s[1:]) for s in streams]
    while any(rest):
        k = int(rng.choice([i for i, r in enumerate(rest) if r]))
        out.append(rest[k].pop(0))
    return out


def head_page(serial, body, flags=2, nseg=None):
    """a first page with this body in one segment, or with nseg segments of no bytes"""
    lacing = [len(body)] if nseg is None else [0] * nseg
    return page(serial, 0, lacing, body, flags)


def sized_page(serial, seq, total, rng, flags=0, mark=False):
    """a page of exactly `total` bytes (27 at least)"""
    nseg = 0 if total == 27 else min(255, max(1, -(-(total - 27) // 256)))
    body = total - 27 - nseg
    lacing = [body // nseg + (1 if i < body % nseg else 0) for i in range(nseg)] if nseg else []
    data = bytearray(random_bytes(rng, body))
    if mark:
        assert body >= 7
        data[:7] = MARK
    return page(serial, seq, lacing, bytes(data), flags)


# ---- what the corpora share --------------------------------------------------------------------------------------------

def random_bytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def corruptions(blob):
    """name -> the valid file `blob` (one with a page that continues a packet) damaged in one way"""
    pages = split_pages(blob)
    j = b"".join
    cont = next(i for i, p in enumerate(pages) if p[5] & 1)            # a page that continues a packet
    out = {}
    bad = bytearray(blob)
    bad[0:4] = b"OggT"
    out["capture pattern"] = bytes(bad)
    out["capture pattern of page 2"] = j(pages[:2]) + b"Ogx" + j(pages[2:])[3:]
    p = [bytearray(x) for x in pages]
    p[1][4] = 1
    out["version"] = j(p[:1] + [recrc(p[1])] + p[2:])
    bad = bytearray(blob)
    bad[len(pages[0]) + 40] ^= 0x10
    out["crc"] = bytes(bad)
    out["truncated page"] = blob[:-1]
    out["truncated header"] = j(pages) + pages[0][:20]
    p = [bytearray(x) for x in pages]
    p[2][14:18] = struct.pack("<I", 999)
    out["second serial"] = j(p[:2] + [recrc(p[2])] + p[3:])
    out["out of sequence"] = j(pages[:2] + pages[3:])
    p = [bytearray(x) for x in pages]
    p[cont][5] &= ~1
    out["continuation without the flag"] = j(p[:cont] + [recrc(p[cont])] + p[cont + 1:])
    out["fewer than three packets"] = j(pages[:1])
    out["empty"] = b""
    return out


def pack(blobs, first=0):
    """`first` bytes of 0xEE, then the files (or chunks) back to back -> (uint8 array, offsets int64 [n + 1])"""
    offsets = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offsets[1:])
    return np.frombuffer(b"\xee" * first + b"".join(blobs), np.uint8), offsets + first


def guarded_mapping(libc, size):
    """an anonymous mapping whose page after `size` bytes (rounded up to pages) is inaccessible"""
    ps = mmap.PAGESIZE
    n = (size + ps - 1) // ps * ps
    m = mmap.mmap(-1, n + ps)
    base = C.addressof(C.c_char.from_buffer(m))
    assert libc.mprotect(C.c_void_p(base + n), C.c_size_t(ps), 0) == 0     # PROT_NONE
    return m, base, n
