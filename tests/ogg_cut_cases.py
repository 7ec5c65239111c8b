"""Shared by test_ogg_cut_cpu.py and test_ogg_cut_gpu.py: the cut rule of csrc/ogg_cut.h as plain Python over an index
(decode_index_scan_host's arrays) and OggStream, the host writer that test_stream_wrapper.py pins; the sources the
cuts are taken from; the windows; and the C calls of the host twin."""
import functools

import numpy as np

from tests.decode_packets import dump_packets, true_granules, with_bad_packets
from tests.ogg_pages import parse_pages, random_bytes

ECAP, ESHAPE = 1, 2
SERIAL = 77                                               # of the sources
DUMPS = {"2ch": (2, 44100, 0.5, "ref_scalar_2ch_44100_q05_20s.pkt", 150),
         "6ch": (6, 48000, 0.8, "ref_scalar_6ch_48000_q08_10s.pkt", 60)}


# ---- sources -----------------------------------------------------------------------------------------------------------

def write(headers, packets, granules, serial=SERIAL):
    """the packets paged as write_ogg pages them, granules[j] on packet j, e_o_s on the last -> .ogg bytes"""
    from vorbis_aotuv_lancer_amd import OggStream
    os_ = OggStream(serial)
    for h in headers:
        os_.packetin(h, 0)
    out = os_.pages(flush=True)
    for j, (p, g) in enumerate(zip(packets, granules)):
        os_.packetin(p, int(g), j == len(packets) - 1)
        out += os_.pages()
    out += os_.pages(flush=True)
    os_.close()
    return b"".join(out)


def pad(packets, size):
    """trailing zero bytes up to `size`: they do not change a packet's decode"""
    return [p + b"\0" * max(0, size - len(p)) for p in packets]


class Source:
    """One stream: .blob (the .ogg file), .headers, its demuxed packets and its index"""

    def __init__(self, name, headers, ds, packets, granules):
        from vorbis_aotuv_lancer_amd import decode_index_scan_host, demux_ogg
        self.name = name
        self.blob = write(headers, packets, granules)
        self.headers, self.data, self.offsets, self.gp, self.eos = demux_ogg(self.blob)
        assert self.headers == list(headers) and len(self.offsets) - 1 == len(packets)
        self.status, self.begin, self.end, self.out_start, totals = decode_index_scan_host(
            ds, self.data, self.offsets, self.gp, self.eos)
        self.total = int(totals[0])
        self.out_end = self.out_start + (self.end - self.begin)
        self.npackets = len(packets)

    @classmethod
    def from_blob(cls, name, blob):
        """the source that an .ogg file is, as it stands"""
        import vorbis_aotuv_lancer_amd as v
        self = cls.__new__(cls)
        self.name, self.blob = name, blob
        self.headers, self.data, self.offsets, self.gp, self.eos = v.demux_ogg(blob)
        ds = v.DecodeSetup(self.headers)
        self.status, self.begin, self.end, self.out_start, totals = v.decode_index_scan_host(
            ds, self.data, self.offsets, self.gp, self.eos)
        ds.close()
        self.total, self.npackets = int(totals[0]), len(self.offsets) - 1
        self.out_end = self.out_start + (self.end - self.begin)
        return self

    def packets(self):
        return [self.packet(j) for j in range(self.npackets)]

    def packet(self, j):
        return self.data[int(self.offsets[j]):int(self.offsets[j + 1])].tobytes()


def from_packets(name, headers, packets, variant="plain"):
    """variant: plain; trim (the last granule lowered by 300); low (the first page's granule lowered by 700: the page
    holds several packets, so its last one begins trimmed after output has begun)"""
    import vorbis_aotuv_lancer_amd as v
    ds = v.DecodeSetup(headers)
    g = true_granules(ds, packets)
    if variant == "trim":
        g[-1] = max(g[-1] - 300, 0)
    if variant == "low":
        gp = v.demux_ogg(write(headers, packets, g))[3]
        first = int(np.flatnonzero(gp != -1)[0])
        assert first >= 3                                 # several packets lie on the first audio page
        g[first] = max(g[first] - 700, 0)
    src = Source(name, headers, ds, packets, g)
    ds.close()
    return src


@functools.lru_cache(maxsize=None)
def dump_source(name):
    """name: "<2ch|6ch>[-<trim|low>][-bad][-pad<size>[x<packets>]]" over the reference's packet dumps"""
    import vorbis_aotuv_lancer_amd as v
    parts = name.split("-")
    ch, rate, q, golden, n = DUMPS[parts[0]]
    headers = v.header_packets(v.Setup(ch, rate, q))
    packets = dump_packets(golden)[:n]
    variant = "plain"
    for p in parts[1:]:
        if p == "bad":
            packets = with_bad_packets(packets, headers, 11)
        elif p.startswith("pad"):
            size, _, count = p[3:].partition("x")
            packets = pad(packets[:int(count)] if count else packets, int(size))
        else:
            variant = p
    return from_packets(name, headers, packets, variant)


def synthetic_source(sizes, seed=3, step=100):
    """Packets of these sizes that no decoder takes, under a made-up index: every packet valid, the first gives nothing,
    every other `step` samples.  For the paging alone."""
    rng = np.random.default_rng(seed)
    src = Source.__new__(Source)
    src.name, src.headers = "synthetic", [b"\x01vorbis-id", b"\x03vorbis-comment", b"\x05vorbis-setup" * 40]
    packets = [random_bytes(rng, n) for n in sizes]
    src.data = np.frombuffer(b"".join(packets), np.uint8).copy()
    src.offsets = np.cumsum([0] + list(sizes)).astype(np.int64)
    P = len(sizes)
    src.status, src.begin = np.zeros(P, np.int32), np.zeros(P, np.int32)
    src.end = np.full(P, step, np.int32)
    src.end[0] = 0
    src.out_end = np.cumsum(src.end).astype(np.int64)
    src.out_start = src.out_end - src.end
    src.total, src.npackets, src.blob = int(src.out_end[-1]), P, None
    return src


class Store:
    """Several sources as the one CSR and index the twin takes"""

    def __init__(self, sources):
        self.sources = list(sources)
        cat = lambda name, dt: np.ascontiguousarray(np.concatenate([getattr(s, name) for s in self.sources]).astype(dt))
        self.first = np.cumsum([0] + [s.npackets for s in self.sources]).astype(np.int64)
        self.status, self.begin = cat("status", np.int32), cat("begin", np.int32)
        self.out_end, self.data = cat("out_end", np.int64), cat("data", np.uint8)
        self.totals = np.array([s.total for s in self.sources], np.int64)
        base = np.cumsum([0] + [len(s.data) for s in self.sources])
        self.offsets = np.concatenate([np.zeros(1, np.int64)] + [s.offsets[1:] + b for s, b in zip(self.sources, base)])
        self.offsets = np.ascontiguousarray(self.offsets, np.int64)

    def index(self):
        return self.first, self.status, self.begin, self.out_end, self.totals, self.data, self.offsets


# ---- the rule ----------------------------------------------------------------------------------------------------------

def find(src, s, L):
    """-> (got, pre, k, m) of the window; (0, ...) for an empty one"""
    got = int(max(0, min(src.total - s, L)))
    if got == 0:
        return 0, -1, -1, -1
    k = int(np.searchsorted(src.out_end, s, side="right"))
    m = int(np.searchsorted(src.out_end, s + got - 1, side="right"))
    pre = k - 1
    while src.status[pre] != 0:
        pre -= 1
    assert pre >= 0
    return got, pre, k, m


def model(src, s, L, serial):
    """The cut of [s, s + L) of the source -> (file bytes, start, length, status, (pre, k, m)); not to be changed"""
    from vorbis_aotuv_lancer_amd import OggStream
    got, pre, k, m = find(src, s, L)
    if got == 0:
        return b"", s, 0, 0, None
    if k == m:                                            # one granule position cannot trim both ends
        got += s - int(src.out_start[k])
        s = int(src.out_start[k])
    refused = (b"", s, 0, ESHAPE, (pre, k, m))
    if any(src.begin[j] != 0 for j in range(k + 1, m + 1)) or (k == m and src.begin[k] != 0):
        return refused                                    # (b), (c)
    os_ = OggStream(serial)
    try:
        for h in src.headers:
            os_.packetin(h, 0)
        out = os_.pages(flush=True)
        gran = lambda j: got if j == m else int(src.out_end[j]) - s
        for j in range(pre, k + 1):
            os_.packetin(src.packet(j), gran(j), j == m)
        first = os_.pages(flush=True)                     # the forced flush: k carries the first granule position
        if len(first) != 1:
            return refused                                # (a)
        out += first
        for j in range(k + 1, m + 1):
            os_.packetin(src.packet(j), gran(j), j == m)
            out += os_.pages()
        assert os_.pages(flush=True) == []                # everything went out at e_o_s
    finally:
        os_.close()
    return b"".join(out), s, got, 0, (pre, k, m)


def check_cut(src, cut, length, pkm, serial):
    """what every non-empty cut of a decodable source must be, whatever made it"""
    import vorbis_aotuv_lancer_amd as v
    pre, k, m = pkm
    headers, data, offsets, gp, eos = v.demux_ogg(cut)
    assert headers == src.headers
    assert [data[int(a):int(b)].tobytes() for a, b in zip(offsets[:-1], offsets[1:])] == [src.packet(j) for j in range(pre, m + 1)]
    assert eos[-1] == 1 and not eos[:-1].any()
    ds = v.DecodeSetup(headers)
    assert v.decode_index(ds, data, offsets, gp, eos)[3] == length
    ds.close()
    pages = parse_pages(cut)
    assert [p["seq"] for p in pages] == list(range(len(pages))) and {p["serial"] for p in pages} == {serial & 0xffffffff}
    assert pages[0]["flags"] == 2 and pages[-1]["flags"] & 4


# ---- windows -----------------------------------------------------------------------------------------------------------

def windows(src, nrandom, seed=5, longest=6000):
    """(s, L) over one source: the directed ones, then nrandom seeded ones"""
    T, oe, os_ = src.total, src.out_end, src.out_start
    n = (src.end - src.begin).astype(np.int64)
    w = [(0, 1), (0, 5000), (0, T), (0, T + 10), (T - 1, 1), (T - 1, 50), (max(0, T - 3000), 3000), (max(0, T - 3000), 9000),
         (T, 10), (T + 5, 10), (T // 2, 0), (T // 3, 1), (T // 2, 1)]
    big = [j for j in range(len(n)) if n[j] >= 100]
    for j in big[:2] + big[len(big) // 2:len(big) // 2 + 2] + big[-2:]:      # inside one packet
        w += [(int(os_[j]) + 10, 20), (int(os_[j]), int(n[j])), (int(os_[j]) + int(n[j]) - 1, 1), (int(os_[j]), 1)]
    change = [j for j in range(2, len(n) - 1) if n[j] and n[j - 1] and n[j] != n[j - 1]]
    for j in change[:6]:                                  # across a short/long transition
        w += [(max(0, int(os_[j]) - 50), 150), (max(0, int(os_[j - 1]) + 1), int(n[j - 1] + n[j] + 5)), (int(oe[j]) - 1, 2)]
    for j in (1, 2, len(n) // 2):                         # exactly on packet boundaries
        w += [(int(os_[j]), int(oe[min(j + 3, len(n) - 1)] - os_[j]))]
    rng = np.random.default_rng(seed)
    for _ in range(nrandom):
        s = int(rng.integers(0, T))
        w.append((s, int(rng.integers(1, longest))))
    return w


# ---- the twin ----------------------------------------------------------------------------------------------------------

def header_pages(store, ranges, serial=0):
    """per range the pages that open its source's file, made under `serial` (the cut writes its own serial number into
    them); None: under the range's serial number, which leaves the cut nothing to rewrite"""
    from vorbis_aotuv_lancer_amd.stream import header_pages as hp
    return [_hp(store.sources[i], sn if serial is None else serial, hp) for i, _, _, sn in ranges]


_HP = {}


def _hp(src, serial, hp):
    key = (id(src), serial)
    if key not in _HP:
        _HP[key] = (src, hp(src.headers, serial))       # the source is kept, so that its id stays its own
    return _HP[key][1]


def run_twin(store, ranges, cap=None, guard=0, header_serial=0):
    """ranges: (stream, s, L, serial).  cap None: one call for the sizes, then one of exactly that capacity.
    header_serial: what the given header pages were made under (header_pages above).
    -> ([bytes], offsets, status [n + 1], starts, lengths, the output buffer with `guard` bytes of 0xa5 behind it)"""
    from vorbis_aotuv_lancer_amd import OggCutter
    pages = header_pages(store, ranges, header_serial)
    ids, st, ln, sn = ([r[c] for r in ranges] for c in range(4))
    hb = sum(len(p) for p in set(pages))
    if cap is None:
        c = OggCutter(max(1, len(ranges)), 0, hb, host=True)
        off = c.cut(store.index(), ids, st, ln, pages, sn)[0]
        c.close()
        cap = int(off[-1])
    c = OggCutter(max(1, len(ranges)), cap, hb, host=True)
    buf = np.full(cap + guard, 0xa5, np.uint8)
    off, stat, gs, gl = c.cut(store.index(), ids, st, ln, pages, sn, out=buf[:cap] if cap else None)
    c.close()
    raw = buf.tobytes()
    outs = [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])] if stat[-1] == 0 else None
    return outs, off, stat, gs, gl, buf


def expected(store, ranges):
    """the model over a call -> ([bytes], offsets, status [n], starts, lengths, [(pre, k, m)])"""
    res = [model(store.sources[i], s, L, serial) for i, s, L, serial in ranges]
    off = np.cumsum([0] + [len(r[0]) for r in res]).astype(np.int64)
    return ([r[0] for r in res], off, np.array([r[3] for r in res], np.int32), np.array([r[1] for r in res], np.int64),
            np.array([r[2] for r in res], np.int64), [r[4] for r in res])
