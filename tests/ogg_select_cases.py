"""Shared by test_ogg_select_cpu.py and test_ogg_select_gpu.py: multiplexed corpora, the rule of csrc/ogg_select.h as a
byte-serial page walker in Python (the first yardstick; the second is vbm_ogg_demux on the Vorbis-only file a
multiplexed one was built from, ogg_demux_batch.single), and the C calls of the selection's host twin and device form
over one interface."""
import functools
import struct

import numpy as np

from tests import ogg_chain_cases as CH
from tests import ogg_demux_batch as B
from tests import ogg_pages as PG
from tests.ogg_demux_batch import ECAP, EINVAL, EOGG  # noqa: F401
from tests.ogg_pages import MARK, corruptions, head_page, interleave, lay, random_bytes, recrc, sized_page
from tests.ogg_twin import Result, Twin

INFO_FIELDS = ("kept_bytes", "kept_pages", "foreign_pages", "streams", "foreign_streams", "first_serial")


def chunk():
    from vorbis_aotuv_lancer_amd.stream import StreamSelector
    return StreamSelector.CHUNK


# ---- the rule ----------------------------------------------------------------------------------------------------------

def model(data):
    """-> (the kept bytes of the file `data`, its info as a dict, its runs [(src, len, dst)]); not to be changed"""
    return _model(bytes(data))


@functools.lru_cache(maxsize=None)
def _model(data):
    end, pos = len(data), 0
    state = PG.GROUP_START
    info = dict.fromkeys(INFO_FIELDS, 0)
    kept = []                                             # (pos, len) of every kept piece, in order
    for p in PG.parse(data, 0, end):
        s = p.serial
        head = bool(p.flags & 2) or pos == 0
        state, picked = PG.group_step(state, head, s, PG.body7(data, p))
        if picked:
            if info["streams"] == 0:
                info["first_serial"] = s
            info["streams"] += 1
        n = p.size
        if state[1] and s == state[2]:
            kept.append((pos, n))
            info["kept_pages"] += 1
        else:
            info["foreign_pages"] += 1
            info["foreign_streams"] += head
        pos += n
    chosen = state[1]
    if chosen and end > pos:
        kept.append((pos, end - pos))
    runs, dst = [], 0
    for at, n in kept:
        if runs and runs[-1][0] + runs[-1][1] == at:
            runs[-1][1] += n
        else:
            runs.append([at, n, dst])
        dst += n
    info["kept_bytes"] = dst
    return b"".join(data[a:a + n] for a, n in kept), info, [tuple(r) for r in runs]


def expected(blobs):
    """-> (out bytes, out_offsets [n + 1], [info dict]) of a batch by the model"""
    outs, infos = [], []
    for b in blobs:
        o, i, _ = model(b)
        outs.append(o)
        infos.append(i)
    off = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(o) for o in outs], out=off[1:])
    return b"".join(outs), off, infos


# ---- streams of pages --------------------------------------------------------------------------------------------------

def foreign(kind, serial, seed, sizes=(40, 300, 9, 700), max_segs=3):
    """a stream that is not Vorbis: random packets behind a plausible first one"""
    rng = np.random.default_rng(seed)
    first = {"skeleton": b"fishead\0" + random_bytes(rng, 56), "theora": b"\x80theora" + random_bytes(rng, 35),
             "opus": b"OpusHead" + random_bytes(rng, 11)}[kind]
    rest = [(b"fisbone\0" if kind == "skeleton" else b"") + random_bytes(rng, n) for n in sizes]
    return lay([first] + rest, serial, max_segs)


def vorbis_pages(k, serial=None):
    """small link k of ogg_chain_cases as pages, under its own serial number or another"""
    blob = CH.small_links(8)[k]
    return PG.split_pages(blob if serial is None else CH.reserial(blob, serial), as_bytes=True)


def _cat(pages):
    return b"".join(pages)


# ---- corpus: name -> (multiplexed file, the Vorbis-only file it must come out as) ---------------------------------------

@functools.lru_cache(maxsize=None)
def case1():
    """Skeleton first; the foreign stream ends before the audio does"""
    v = vorbis_pages(4)
    sk = foreign("skeleton", 71, 1, sizes=(80, 600, 80))
    pages = [sk[0], v[0]] + sk[1:] + v[1:]
    assert pages[-1] == v[-1] and sk[-1][5] & 4
    return {"skeleton first": (_cat(pages), _cat(v))}


@functools.lru_cache(maxsize=None)
def case2():
    """video-like: pages of 255 segments and 65025 body bytes, packets continued over pages, audio in between"""
    v = vorbis_pages(3)
    th = foreign("theora", 72, 2, sizes=(150000, 30, 66000), max_segs=255)
    assert sum(1 for p in th if p[26] == 255 and len(p) == 27 + 255 + 65025) >= 2 and any(p[5] & 1 for p in th)
    return {"video-like": (_cat(interleave([th, v], 3)), _cat(v))}


@functools.lru_cache(maxsize=None)
def case3():
    v = vorbis_pages(2)
    out = {"vorbis head first": (_cat(interleave([v, foreign("theora", 73, 4)], 5)), _cat(v))}
    three = [foreign("skeleton", 74, 6), v, foreign("theora", 75, 7), foreign("opus", 76, 8)]
    out["three foreign streams around one"] = (_cat(interleave(three, 9)), _cat(v))
    return out


@functools.lru_cache(maxsize=None)
def case4():
    a, b = vorbis_pages(4), vorbis_pages(3)
    return {"two vorbis streams": (_cat(interleave([a, b], 10)), _cat(a)),
            "two vorbis streams behind a foreign one": (_cat(interleave([foreign("skeleton", 77, 11), b, a], 12)), _cat(b))}


@functools.lru_cache(maxsize=None)
def case5():
    """chained multiplexed files; the second element is the plain chain of the chosen links"""
    a, b, c = vorbis_pages(4), vorbis_pages(3), vorbis_pages(2)
    sa = struct.unpack_from("<I", a[0], 14)[0]
    g1 = interleave([foreign("skeleton", 80, 13), a], 14)
    # group 2: its Vorbis stream has another serial, a foreign one reuses group 1's foreign serial, and another foreign
    # one runs under the serial group 1 chose
    g2 = interleave([foreign("theora", 80, 15), foreign("opus", sa, 16), b], 17)
    g3 = interleave([c, foreign("theora", 81, 18)], 19)
    none = interleave([foreign("theora", 82, 20), foreign("opus", 83, 21)], 22)
    out = {"two groups": (_cat(g1 + g2), _cat(a + b)),
           "three groups": (_cat(g1 + g2 + g3), _cat(a + b + c)),
           "a group without vorbis in the middle": (_cat(g1 + none + g3), _cat(a + c))}
    assert struct.unpack_from("<I", b[0], 14)[0] != sa
    return out


@functools.lru_cache(maxsize=None)
def case6():
    """no Vorbis stream anywhere: nothing is kept"""
    return {"foreign alone": _cat(foreign("theora", 84, 23)),
            "opus-like": _cat(foreign("opus", 85, 24)),
            "two foreign streams": _cat(interleave([foreign("skeleton", 86, 25), foreign("theora", 87, 26)], 27))}


@functools.lru_cache(maxsize=None)
def case7():
    """plain files and plain chains: out as they went in"""
    out = {f"link {k}": blob for k, blob in enumerate(CH.small_links(3))}
    # not plain: "multiplexed start" is two streams, and the group that "flag on a later page" starts shows no mark
    out.update({name: blob for name, (blob, _) in CH.chains().items()
                if name not in ("multiplexed start", "flag on a later page")})
    return out


@functools.lru_cache(maxsize=None)
def case8():
    """edges (zero files is a batch of its own)"""
    v = vorbis_pages(4)
    tail = v[1:]
    plain = _cat(v)
    noflag = bytearray(v[0])
    noflag[5] &= ~2
    noflag = bytes(recrc(noflag))
    other = bytearray(noflag)
    other[27 + other[26]] = 3                               # the packet type byte: no mark
    other = bytes(recrc(other))
    return {"empty": b"", "1 byte": plain[:1], "26 bytes": plain[:26], "27 bytes": plain[:27],
            "head page of no segments": _cat([head_page(90, b"", nseg=0)] + v),
            "head page with a body of 6": _cat([head_page(91, MARK[:6])] + tail),
            "head page with a body of exactly 7": _cat([head_page(struct.unpack_from("<I", v[0], 14)[0], MARK)] + tail),
            "body of 7, one byte wrong": _cat([head_page(92, b"\x01vorbit")] + tail),
            "first page without the flag, with the mark": _cat([noflag] + tail),
            "first page without the flag or the mark": _cat([other] + tail)}


def singles():
    """every (name, multiplexed file, Vorbis-only file) of cases 1 to 5"""
    out = [(name, m, want) for case in (case1, case2, case3, case4, case5) for name, (m, want) in case().items()]
    assert len(out) == N_SINGLES
    return out


@functools.lru_cache(maxsize=None)
def damage():
    """every corruptions variant of cases 1, 2 and 5"""
    out = {}
    for src in (case1()["skeleton first"][0], case2()["video-like"][0], case5()["three groups"][0]):
        for name, bad in corruptions(src).items():
            out[f"{len(out)} {name}"] = bad
    return out


@functools.lru_cache(maxsize=None)
def cuts():
    """one multiplexed file of about 3 KB cut at every length from 0 to its size"""
    blob = _cat(interleave([vorbis_pages(0), foreign("theora", 88, 28, sizes=(40, 60))], 29))
    assert 3000 < len(blob) < 4500, len(blob)               # the setup header alone is 3 KB
    return [blob[:n] for n in range(len(blob) + 1)]


@functools.lru_cache(maxsize=None)
def alignment_files():
    """files whose kept runs are single pages of 27 to 27 + 64 bytes (bodies of 0 to 40 bytes and a few more) between
    foreign pages of varied sizes: every run length, and with the batch's first byte at 0 to 15 every pair of (source,
    destination) alignments"""
    rng = np.random.default_rng(31)
    files = []
    for f in range(6):
        pages = [sized_page(500, 0, 27 + 1 + 30, rng, 2, mark=True), sized_page(600, 0, 27 + int(rng.integers(0, 50)), rng, 2)]
        lengths = list(rng.permutation(np.arange(27, 27 + 65)))
        for k, n in enumerate(lengths):
            pages.append(sized_page(600, k + 1, 27 + int(rng.integers(0, 70)), rng))
            pages.append(sized_page(500, k + 1, int(n), rng))
        files.append(_cat(pages) + b"\x00" * f)              # a kept tail of 0 to 5 bytes behind the last kept page
    return files


def alignment_coverage(files):
    """-> ({(source mod 16, destination mod 16) of the run starts over first = 0 .. 15}, {run lengths})"""
    pairs, lengths, src0, dst0 = set(), set(), 0, 0
    for b in files:
        out, _, runs = model(b)
        for src, n, dst in runs:
            lengths.add(n)
            pairs |= {((first + src0 + src) % 16, (dst0 + dst) % 16) for first in range(16)}
        src0 += len(b)
        dst0 += len(out)
    return pairs, lengths


@functools.lru_cache(maxsize=None)
def chunk_files():
    """runs of CHUNK - 1, CHUNK and CHUNK + 1 bytes, one run over three chunks, and a file of more runs than a wavefront
    has lanes"""
    rng = np.random.default_rng(32)
    K = chunk()

    def run(seq, total, mark=False):
        if mark:
            return [sized_page(500, seq, 58, rng, 2, mark=True), sized_page(500, seq + 1, total - 58, rng)]
        return [sized_page(500, seq, total, rng)]

    pages = [sized_page(600, 0, 100, rng, 2)] + run(0, K - 1, mark=True)
    for k, total in enumerate((K, K + 1, 3 * K + 100)):
        pages += [sized_page(600, k + 1, 33 + k, rng)] + run(k + 2, total)
    edges = _cat(pages + [sized_page(600, 4, 37, rng, 4)])
    many = [sized_page(500, 0, 58, rng, 2, mark=True)]
    for k in range(70):
        many += [sized_page(600, k, 27 + k % 9, rng, 2 if k == 0 else 0), sized_page(500, k + 1, 40 + k, rng)]
    many = _cat(many)
    assert sorted(r[1] for r in model(edges)[2]) == [K - 1, K, K + 1, 3 * K + 100] and len(model(many)[2]) == 71
    return [edges, many]


GROUPS = ("cases 1 to 5", "no vorbis", "identity", "edges", "zero files", "damage", "cuts", "chunk edges", "alignment")
N_SINGLES = 9


def group(name):
    """-> [blobs]: the corpus as the batches the tests run, built when asked for"""
    return {"cases 1 to 5": lambda: [m for _, m, _ in singles()],
            "no vorbis": lambda: list(case6().values()),
            "identity": lambda: list(case7().values()),
            "edges": lambda: list(case8().values()),
            "zero files": lambda: [],
            "damage": lambda: list(damage().values()),
            "cuts": cuts,
            "chunk edges": chunk_files,
            "alignment": alignment_files}[name]()


# ---- the host twin and the device calls (ogg_twin.Twin) ------------------------------------------------------------------

def info_dtype():
    from vorbis_aotuv_lancer_amd.stream import SELECT_INFO
    return SELECT_INFO


class Select(Twin):
    """A selector and its buffers"""

    GUARD = 64

    def __init__(self, impl, max_files, max_bytes):
        super().__init__(impl, "select", max_files, max_bytes)

    def select_raw(self, nfiles, data_ptr, off_ptr, out_ptr, out_cap, out_off_ptr, info_ptr):
        return self.call("select", nfiles, data_ptr, off_ptr, out_ptr, out_cap, out_off_ptr, info_ptr)

    def select(self, data, offsets, out_cap):
        """data: uint8 numpy or an address -> Result: .out [out_cap], .out_offsets [n + 1], .info [n], .status, .touched
        (out differs from its blank pattern), .guard_ok (GUARD bytes behind out and behind each small output)"""
        n = len(offsets) - 1
        if isinstance(data, np.ndarray):
            data = self.upload(data)
        isz, g = info_dtype().itemsize, self.GUARD
        out, oo, info = (self.guarded(k, np.uint8, g) for k in (out_cap, 8 * (n + 1), n * isz))
        off = np.ascontiguousarray(offsets, np.int64)
        rc = self.select_raw(n, data, off.ctypes.data, self.ptr(out), out_cap, self.ptr(oo), self.ptr(info))
        assert rc == 0, (rc, self.lib.vbm_last_error())
        r = Result()
        r.status = self.status()
        (r.out, r.touched, ok0), (oo, _, ok1), (info, _, ok2) = (self.unguard(a, k) for a, k in
                                                                 ((out, out_cap), (oo, 8 * (n + 1)), (info, n * isz)))
        r.guard_ok = ok0 and ok1 and ok2
        r.out_offsets, r.info = oo.copy().view(np.int64), info.copy().view(info_dtype())
        return r


def run(impl, blobs, first=0, out_cap=None):
    """the selection of one batch whose first file starts at byte `first`, into a buffer of exactly the kept total (or
    out_cap) -> Result, with .out cut to the total"""
    data, offsets = B.pack(blobs, first)
    total = sum(len(model(b)[0]) for b in blobs)
    s = Select(impl, max(1, len(blobs)), int(offsets[-1] - offsets[0]))
    try:
        r = s.select(data, offsets, total if out_cap is None else out_cap)
    finally:
        s.close()
    assert r.status == 0 and r.guard_ok, (r.status, r.guard_ok)
    r.out = r.out[:total]
    return r


def same_info(info, want):
    """the records of a batch equal the model's dicts"""
    for f, w in enumerate(want):
        for name in INFO_FIELDS:
            assert int(info[name][f]) == w[name], (f, name, int(info[name][f]), w[name])
        assert int(info["reserved"][f]) == 0
    return True


def check_model(impl, blobs, first=0, out_cap=None):
    """the selection equals the model's -> Result"""
    r = run(impl, blobs, first, out_cap)
    want_out, want_off, want_info = expected(blobs)
    assert np.array_equal(r.out_offsets, want_off), (r.out_offsets, want_off)
    assert r.out.tobytes() == want_out
    assert same_info(r.info, want_info)
    return r


def check_twin(blobs, first=0, out_cap=None):
    """the device form equals the host twin, byte for byte -> the device's Result"""
    h, d = run("host", blobs, first, out_cap), run("device", blobs, first, out_cap)
    assert np.array_equal(d.out_offsets, h.out_offsets)
    assert np.array_equal(d.out, h.out)
    assert d.info.tobytes() == h.info.tobytes()
    return d
