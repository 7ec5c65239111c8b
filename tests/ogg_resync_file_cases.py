"""Shared by test_ogg_resync_files_cpu.py, test_ogg_resync_files_gpu.py and test_decode_resync_files_gpu.py: whole files
that are damaged, chained or both, the yardstick (tests/ogg_resync_model.py: run(blob) with no cuts and end, then the
links that completed three headers, and the sums of its call records), and a driver over ResyncDemuxer.demux_joined (host
twin or device) that returns a batch in the yardstick's form."""
import functools

import numpy as np

from tests import ogg_chain_cases as CH
from tests import ogg_feed_resync_cases as RC
from tests import ogg_resync_model as M
from tests.ogg_pages import pack, page, random_bytes

ECAP, EINVAL = 1, -131
JUNK = (1, 3, 4, 27, 300)
EVENTS = ("links_started", "links_bad", "gaps", "skipped_bytes", "ignored_pages", "pages")


# ---- the yardstick -----------------------------------------------------------------------------------------------------

class _Counting(M.Slot):
    """counts the pages that went by, ignored by rule 2 or taken"""

    def __init__(self):
        super().__init__()
        self.went_by = 0

    def passed(self):
        self.went_by += 1


@functools.lru_cache(maxsize=None)
def model_file(blob):
    """-> ([(headers [3], [(bytes, granulepos, eos, gap)])] per entry, {event: count}) of one file pushed whole with end"""
    slot, calls = M.run(blob, slot=_Counting())
    entries = [(l.headers, list(zip(l.packets, l.granulepos, l.eos, l.gap))) for l in slot.links if len(l.headers) == 3]
    ignored = sum(c["ignored"] for c in calls)
    ev = {"links_started": len(slot.links), "links_bad": len(slot.links) - len(entries),
          "gaps": sum(c["gaps"] for c in calls), "skipped_bytes": sum(c["skipped"] for c in calls),
          "ignored_pages": ignored, "pages": slot.went_by - ignored}
    assert ev["links_started"] == sum(c["link_started"] for c in calls)
    return entries, ev


# ---- driver ------------------------------------------------------------------------------------------------------------

def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def make(impl, nfiles, nbytes, **kw):
    import vorbis_aotuv_lancer_amd as v
    return v.ResyncDemuxer(max(1, nfiles), nbytes, host=impl == "host", **kw)


def run(impl, blobs, first=0, rd=None, entry_cap=None, **kw):
    """the files as one batch that starts `first` bytes into its buffer -> DemuxBatch"""
    raw, off = pack(blobs, first)
    own = rd or make(impl, len(blobs), int(off[-1] - off[0]), **kw)
    try:
        if not own.host:
            import torch
            raw = torch.from_numpy(raw.copy()).to(own.device)
        return own.demux_joined([f"f{i}" for i in range(len(blobs))], raw, off, entry_cap=entry_cap)
    finally:
        if rd is None:
            own.close()


def file_result(b, f, arrays=None):
    """given file f of a batch, in model_file's form"""
    pay, offs, gp, eos, gap = arrays or batch_arrays(b)
    entries = []
    for k, e in enumerate(b.links(f)):
        fi = b.info[e]
        a, n = int(fi["packet_base"]), int(fi["packets"])
        assert fi["status"] == 0 and b.names[e] == f"f{f} link {k}"
        assert int(offs[a]) == int(fi["payload_base"]) and int(offs[a + n] - offs[a]) == int(fi["payload_bytes"])
        assert [len(h) for h in b.headers[e]] == fi["header_bytes"].tolist()
        pk = [(pay[int(offs[a + i]):int(offs[a + i + 1])].tobytes(), int(gp[a + i]), int(eos[a + i]), int(gap[a + i]))
              for i in range(n)]
        assert b.gaps(e).shape[0] == n and len(b.runs(e)[1]) == n
        entries.append((b.headers[e], pk))
    return entries, {k: int(b.events[f][k]) for k in EVENTS}


def batch_arrays(b):
    return tuple(_np(x) for x in (b.payload, b.offsets, b.granulepos, b.eos, b.gap))


def batch_bytes(b):
    """everything a batch holds, as bytes: for the device-against-twin comparison"""
    return (b.info.tobytes(), b.events.tobytes(), np.asarray(b.file_links).tobytes(), repr(b.headers).encode(),
            tuple(b.names)) + tuple(x.tobytes() for x in batch_arrays(b))


def check(b, blobs):
    """every file of the batch equals the model: entries, headers, packets, granule positions, eos, marks, events"""
    assert len(b.file_links) == len(blobs) + 1 and len(b) == int(b.file_links[-1]) and b.select_info is None
    arrays = batch_arrays(b)
    assert int(arrays[1][0]) == 0 and len(arrays[1]) == len(arrays[2]) + 1 == len(arrays[4]) + 1
    for f, blob in enumerate(blobs):
        got, want = file_result(b, f, arrays), model_file(bytes(blob))
        assert got[1] == want[1], (f, got[1], want[1])
        assert len(got[0]) == len(want[0]), (f, len(got[0]), len(want[0]))
        for k, (g, w) in enumerate(zip(got[0], want[0])):
            assert g[0] == w[0], (f, k, "headers")
            assert g[1] == w[1], (f, k, len(g[1]), len(w[1]), [i for i, (x, y) in enumerate(zip(g[1], w[1])) if x != y][:4])
    return b


def check_each_and_together(impl, blobs, firsts=(0,)):
    """as one batch in one call, and each file alone (through one object)"""
    blobs = [bytes(x) for x in blobs]
    for first in firsts:
        check(run(impl, blobs, first), blobs)
    rd = make(impl, 1, max(len(x) for x in blobs))
    try:
        for x in blobs:
            check(run(impl, [x], rd=rd), [x])
    finally:
        rd.close()


# ---- corpora: undamaged, and the damage of the feed corpus -------------------------------------------------------------

def undamaged():
    return [b for _, b in RC.good_files()], list(RC.chain_files().values())


def removals(blob):
    """[(the file without one audio page or an adjacent pair, the packets that must survive)]"""
    ap = RC.audio_pages(blob)
    drops = [{k} for k in ap] + [{a, b} for a, b in zip(ap[:-1], ap[1:])]
    return [(RC.without_pages(blob, d), RC.survivors(blob, d)) for d in drops]


def flips(blob):
    out = [RC.flip(blob, k, where) for k in range(len(RC.pages(blob))) for where in ("header", "lacing", "body")]
    return [x for x in out if x is not None]


def junked(blob):
    """1, 3, 4, 27 and 300 bytes of junk at every page boundary, in front of the file and behind it"""
    ps = RC.pages(blob)
    rng = np.random.default_rng(3)
    out = []
    for n in JUNK:
        for k in range(len(ps) + 1):
            junk = random_bytes(rng, n).replace(b"O", b"o")
            out.append(RC.join(ps[:k]) + junk + RC.join(ps[k:]))
    return out


def feed_damage():
    """the false header, the overclaim, a page lost while the headers are open, foreign serials, pages after eos"""
    six, ps = RC.paged_six(), RC.pages(RC.paged_six())
    a, b, c = CH.small_links(3)
    foreign = RC.pages(CH.reserial(six, 555))
    return {"false capture": RC.false_capture_file()[0], "overclaim": RC.overclaim_file()[0],
            "headers open, then a link": ps[0] + RC.join(ps[2:]) + b,
            "headers open, alone": ps[0] + RC.join(ps[2:]),
            "foreign serials": RC.join(ps[:3]) + foreign[4] + RC.join(ps[3:]) + foreign[5] + ps[-1],
            "pages after eos": six + ps[-2] + ps[-1] + foreign[3],
            "chain with a hole in each link": RC.without_pages(a, {3}) + RC.without_pages(b, {2}) + c,
            "mid-page join": six[len(ps[0]) + 10:] + b}


# ---- inputs new here ---------------------------------------------------------------------------------------------------

def tiny():
    return [b"", b"O", b"Og", b"Ogg", b"OggS", b"\0", b"\0\0\0\0", b"OggS\0", b"OggS\1"]


def cut_headers():
    """a page header cut at 5, 26, 27 and 27 + nseg - 1 bytes, behind a good file and alone"""
    six, ps = RC.paged_six(), RC.pages(RC.paged_six())
    p = ps[RC.audio_pages(six)[3]]                       # 600 bytes: three segments
    assert p[26] >= 2
    cuts = (5, 26, 27, 27 + p[26] - 1)
    return [six + p[:c] for c in cuts] + [p[:c] for c in cuts]


def across_boundary():
    """pairs of neighbours whose joined bytes form the capture pattern across the boundary, at each of the three splits"""
    six, (a,) = RC.paged_six(), CH.small_links(1)
    out = []
    for k in (1, 2, 3):
        out += [six + a[:k], a[k:]]
    return out


def shifted():
    """a good file behind 0..7 bytes that are no page"""
    return [b"\x55" * k + RC.paged_six() for k in range(8)]


def straddle_positions():
    """where a capture pattern must start to straddle each boundary of the device's search (all four splits of it, the
    pattern's first byte on the boundary included), in bytes from an aligned buffer start; the grid's: gpu only"""
    import vorbis_aotuv_lancer_amd as v
    R = v.ResyncDemuxer
    base = 2 * R.TILE                                    # behind the headers
    edges = {"dword": base + 4 * 5, "lane": base + R.LANE * 3, "wave": base + R.WAVE * 3, "row": base + R.ROW,
             "tile": base + R.TILE}
    sizes = [4, R.LANE, R.WAVE, R.ROW, R.TILE]
    for k, e in enumerate(edges.values()):               # an edge of its own kind and of no larger one
        assert e % sizes[k] == 0 and (k == 4 or e % sizes[k + 1] != 0)
    return edges


def straddle_file(at, size=None):
    """the headers of paged_six, filler, and its audio pages from byte `at` on, padded to a whole number of tiles (so
    that in a batch of such files every file starts on a tile edge)"""
    import vorbis_aotuv_lancer_amd as v
    six, ps = RC.paged_six(), RC.pages(RC.paged_six())
    ap = RC.audio_pages(six)
    head = RC.join(ps[:ap[0]])
    assert len(head) <= at
    blob = head + b"\x55" * (at - len(head)) + RC.join(ps[ap[0]:])
    tile = v.ResyncDemuxer.TILE
    return blob + b"\x55" * (-len(blob) % tile if size is None else size - len(blob))


def straddles():
    return [straddle_file(e - d) for e in straddle_positions().values() for d in (3, 2, 1, 0)]


def nested():
    """a whole good page stored as the payload of a packet inside a good page, and the same with the outer page's CRC
    broken: the inner page is then met by the walk, foreign (ignored) or the stream's own next page (taken)"""
    rng = np.random.default_rng(21)
    six_pages = RC.pages(RC.paged_six())
    foreign = six_pages[RC.audio_pages(RC.paged_six())[0]]
    out = []
    for own in (False, True):
        # the outer stream's audio pages are numbered from 3 on (RC._mux: three header pages or fewer; found below)
        probe = RC._mux([b"x"], 77, lambda k: True)
        seq0 = len(RC.pages(probe)) - 1
        inner = page(77, seq0 + 1, [10], random_bytes(rng, 10), 0, 999) if own else foreign
        pk = [random_bytes(rng, 40), b"ab" + inner + b"cd", random_bytes(rng, 60)]
        blob = RC._mux(pk, 77, lambda k: True)
        k = RC.audio_pages(blob)[1]
        assert inner in RC.pages(blob)[k]
        out += [blob, RC.flip(blob, k, "header")]
    return out


def edge_claims():
    """a good page whose claim ends exactly at the file's end and one byte past it; one beginning-of-stream page; three
    headers and no audio; three headers in front of a second link"""
    six, ps = RC.paged_six(), RC.pages(RC.paged_six())
    ap = RC.audio_pages(six)
    (a,) = CH.small_links(1)
    return [six, six[:-1], ps[0], RC.join(ps[:ap[0]]), RC.join(ps[:ap[0]]) + a, ps[0] + a]


def sixty_five():
    links = CH.small_links(65)
    return [links[k] + links[(k + 1) % 65] if k % 3 == 0 else RC.without_pages(links[k], {2}) if k % 3 == 1 else links[k]
            for k in range(65)]


def many_candidates():
    """more capture patterns than a small max_candidates: 200 that are no page, then a good file"""
    return b"OggS" * 200 + RC.paged_six()
