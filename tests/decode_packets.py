"""Host-side toolkit of the decoder tests (numpy only, no device): packet lists and their CSR forms, the header
unpacker, the setups and corpora that several test files share, and one restatement of the reference's
vorbis_synthesis_blockin bookkeeping (`blockin`).  The package is imported inside the functions that need it; the
device-side driver is tests/decode_calls.py."""
import functools
import glob
import os
import re
import sys

import numpy as np

from tests import vorbis_model as vm
from tests.encode_oracle import walk
from tests.signals import burst_signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
import vpk  # noqa: E402

DATA = os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "data")
G = os.path.join(ROOT, "tests", "golden")
PACKS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(DATA, "mode_*.vpk")))
NAMES = [name for name, _ in vm.CORPUS]

# the codes vorbis_aotuv_lancer_amd.decoder does not define (include/vorbis_mi355x.h)
EIMPL, EINVAL, ENODEV = -130, -131, -1000
_DECODER_CODES = ("ENOTVORBIS", "EBADHEADER", "EVERSION", "ENOTAUDIO", "EBADPACKET")


def __getattr__(name):
    """the decoder's own error codes, from where the package defines them"""
    if name in _DECODER_CODES:
        from vorbis_aotuv_lancer_amd import decoder
        return getattr(decoder, name)
    raise AttributeError(name)


# the reference encoder's packet dumps in tests/golden: (channels, rate, quality, file)
DUMPS = [(2, 44100, 0.5, "ref_scalar_2ch_44100_q05_20s.pkt"), (6, 48000, 0.8, "ref_scalar_6ch_48000_q08_10s.pkt")]
# the shipped classes of the index tests
INDEX_PACKS = ["mode_1ch_44100_q0.5.vpk", "mode_2ch_44100_q0.1.vpk", "mode_2ch_96000_q0.5.vpk", "mode_1ch_8000_q0.5.vpk",
               "mode_6ch_48000_q0.5.vpk", "mode_2ch_44100_q-0.1.vpk"]
# (channels, rate, quality): the classes of the unpack parity test
PARITY = [(2, 44100, 0.5), (2, 44100, 0.1), (6, 48000, 0.8), (1, 44100, 0.5), (8, 44100, 0.5), (2, 96000, 0.5)]

# the reference's codebook self-test (lib/sharedbook.c:474-610), books 4 and 5
Q_MIN, Q_DELTA = -533200896, 1611661312          # lib/sharedbook.c:513, :524, :535, :554
QUANTLIST = [0, 7, 2]                            # partial_quantlist1, :492
# test4_result (:539-547): entry e, component k -> quantlist[(e / 3^k) % 3] * delta + min, non-sequential
TEST4 = [-3, -3, -3, 4, -3, -3, -1, -3, -3, -3, 4, -3, 4, 4, -3, -1, 4, -3, -3, -1, -3, 4, -1, -3, -1, -1, -3,
         -3, -3, 4, 4, -3, 4, -1, -3, 4, -3, 4, 4, 4, 4, 4, -1, 4, 4, -3, -1, 4, 4, -1, 4, -1, -1, 4,
         -3, -3, -1, 4, -3, -1, -1, -3, -1, -3, 4, -1, 4, 4, -1, -1, 4, -1, -3, -1, -1, 4, -1, -1, -1, -1, -1]
# test5_result (:558-566): the same book with q_sequencep = 1 (running sums along the dimension)
TEST5 = [-3, -6, -9, 4, 1, -2, -1, -4, -7, -3, 1, -2, 4, 8, 5, -1, 3, 0, -3, -4, -7, 4, 3, 0, -1, -2, -5,
         -3, -6, -2, 4, 1, 5, -1, -4, 0, -3, 1, 5, 4, 8, 12, -1, 3, 7, -3, -4, 0, 4, 3, 7, -1, -2, 2,
         -3, -6, -7, 4, 1, 0, -1, -4, -5, -3, 1, 0, 4, 8, 7, -1, 3, 2, -3, -4, -5, 4, 3, 2, -1, -2, -3]


# ---- the header unpacker: the reference's decode side restated (see tests/test_stream_wrapper.py) -------------------
class BitReader:
    """oggpack_read: LSb first"""

    def __init__(self, data):
        self.d, self.pos = data, 0

    def read(self, bits):
        v = 0
        for i in range(bits):
            byte = self.pos >> 3
            if byte >= len(self.d):
                raise EOFError
            v |= ((self.d[byte] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def bytes_left(self):
        return len(self.d) - ((self.pos + 7) >> 3)


def ilog(v):
    return int(v).bit_length()


def maptype1_quantvals(entries, dim):
    vals = max(int(np.floor(np.float32(entries) ** (np.float32(1.) / np.float32(dim)))), 1)
    while True:
        acc, acc1, ok = 1, 1, True
        for _ in range(dim):
            if entries // vals < acc:
                ok = False
                break
            acc *= vals
            acc1 *= vals + 1
        if ok and acc <= entries and acc1 > entries:
            return vals
        vals += -1 if (not ok or acc > entries) else 1


def unpack_book(r):
    assert r.read(24) == 0x564342
    dim, entries = r.read(16), r.read(24)
    assert ilog(dim) + ilog(entries) <= 24
    if r.read(1) == 0:
        unused = r.read(1)
        lengths = []
        for _ in range(entries):
            if unused:
                lengths.append(r.read(5) + 1 if r.read(1) else 0)
            else:
                lengths.append(r.read(5) + 1)
    else:
        length = r.read(5) + 1
        lengths = []
        while len(lengths) < entries:
            num = r.read(ilog(entries - len(lengths)))
            assert length <= 32 and num <= entries - len(lengths)
            lengths += [length] * num
            length += 1
    book = {"dim": dim, "entries": entries, "lengthlist": lengths, "maptype": r.read(4)}
    if book["maptype"] in (1, 2):
        book["q_min"], book["q_delta"] = r.read(32), r.read(32)
        book["q_quant"], book["q_sequencep"] = r.read(4) + 1, r.read(1)
        qv = maptype1_quantvals(entries, dim) if book["maptype"] == 1 else entries * dim
        book["quantlist"] = [r.read(book["q_quant"]) for _ in range(qv)]
    else:
        assert book["maptype"] == 0
    return book


def unpack_headers(h0, h1, h2):
    out = {}
    r = BitReader(h0)
    assert r.read(8) == 1 and bytes(r.read(8) for _ in range(6)) == b"vorbis"
    assert r.read(32) == 0
    out["channels"], out["rate"] = r.read(8), r.read(32)
    out["bitrates"] = [r.read(32), r.read(32), r.read(32)]
    out["blocksizes"] = [1 << r.read(4), 1 << r.read(4)]
    assert r.read(1) == 1 and out["rate"] >= 1 and out["channels"] >= 1 and 64 <= out["blocksizes"][0] <= out["blocksizes"][1] <= 8192
    assert len(h0) == 30

    r = BitReader(h1)
    assert r.read(8) == 3 and bytes(r.read(8) for _ in range(6)) == b"vorbis"
    out["vendor"] = bytes(r.read(8) for _ in range(r.read(32)))
    out["comments"] = [bytes(r.read(8) for _ in range(r.read(32))) for _ in range(r.read(32))]
    assert r.read(1) == 1

    r = BitReader(h2)
    assert r.read(8) == 5 and bytes(r.read(8) for _ in range(6)) == b"vorbis"
    out["books"] = [unpack_book(r) for _ in range(r.read(8) + 1)]
    nb = len(out["books"])
    for _ in range(r.read(6) + 1):          # time backend placeholders
        assert r.read(16) == 0
    floors = []
    for _ in range(r.read(6) + 1):
        assert r.read(16) == 1             # floor type 1
        f = {"partitions": r.read(5)}
        f["partitionclass"] = [r.read(4) for _ in range(f["partitions"])]
        maxclass = max(f["partitionclass"], default=-1)
        f["class_dim"], f["class_subs"], f["class_book"], f["class_subbook"] = [], [], [], []
        for _ in range(maxclass + 1):
            f["class_dim"].append(r.read(3) + 1)
            f["class_subs"].append(r.read(2))
            f["class_book"].append(r.read(8) if f["class_subs"][-1] else None)
            assert f["class_book"][-1] is None or f["class_book"][-1] < nb
            f["class_subbook"].append([r.read(8) - 1 for _ in range(1 << f["class_subs"][-1])])
            assert all(-1 <= x < nb for x in f["class_subbook"][-1])
        f["mult"] = r.read(2) + 1
        rangebits = r.read(4)
        count = sum(f["class_dim"][c] for c in f["partitionclass"])
        assert count <= 63
        f["postlist"] = [0, 1 << rangebits] + [r.read(rangebits) for _ in range(count)]
        assert len(set(f["postlist"])) == len(f["postlist"])   # no repeated posts (zero-length segments)
        floors.append(f)
    out["floors"] = floors
    residues = []
    for _ in range(r.read(6) + 1):
        res = {"type": r.read(16)}
        assert res["type"] in (0, 1, 2)
        res["begin"], res["end"], res["grouping"] = r.read(24), r.read(24), r.read(24) + 1
        res["partitions"], res["groupbook"] = r.read(6) + 1, r.read(8)
        res["secondstages"] = []
        for _ in range(res["partitions"]):
            cascade = r.read(3)
            if r.read(1):
                cascade |= r.read(5) << 3
            res["secondstages"].append(cascade)
        res["booklist"] = [r.read(8) for _ in range(sum(bin(c).count("1") for c in res["secondstages"]))]
        assert res["groupbook"] < nb and all(b < nb and out["books"][b]["maptype"] != 0 for b in res["booklist"])
        gb = out["books"][res["groupbook"]]
        assert gb["dim"] >= 1 and res["partitions"] ** gb["dim"] <= gb["entries"]
        residues.append(res)
    out["residues"] = residues
    maps = []
    ch = out["channels"]
    for _ in range(r.read(6) + 1):
        assert r.read(16) == 0
        m = {"submaps": r.read(4) + 1 if r.read(1) else 1}
        m["coupling"] = []
        if r.read(1):
            for _ in range(r.read(8) + 1):
                mag, ang = r.read(ilog(ch - 1)), r.read(ilog(ch - 1))
                assert mag != ang and mag < ch and ang < ch
                m["coupling"].append((mag, ang))
        assert r.read(2) == 0
        m["chmuxlist"] = [r.read(4) for _ in range(ch)] if m["submaps"] > 1 else [0] * ch
        assert all(x < m["submaps"] for x in m["chmuxlist"])
        m["floorsubmap"], m["residuesubmap"] = [], []
        for _ in range(m["submaps"]):
            r.read(8)
            m["floorsubmap"].append(r.read(8))
            m["residuesubmap"].append(r.read(8))
            assert m["floorsubmap"][-1] < len(floors) and m["residuesubmap"][-1] < len(residues)
        maps.append(m)
    out["maps"] = maps
    modes = []
    for _ in range(r.read(6) + 1):
        md = (r.read(1), r.read(16), r.read(16), r.read(8))
        assert md[1] == 0 and md[2] == 0 and md[3] < len(maps)
        modes.append(md)
    out["modes"] = modes
    assert r.read(1) == 1                      # framing bit
    assert r.bytes_left() == 0                 # nothing but padding bits after it
    return out


# ---- setups and the packets of shipped classes -------------------------------------------------------------------
def pack_setup(v, pack):
    d = vpk.read_vpk(os.path.join(DATA, pack))
    ch, rate, q = int(d["info/channels"][0]), int(d["info/rate"][0]), float(d["info/quality"][0])
    if int(d["info/managed"][0]):
        av, mn, mx, _ = [int(x) for x in d["bi/rates"]]
        return v.Setup(ch, rate, bitrate=(mx, av, mn)), d
    return v.Setup(ch, rate, q), d


def headers_of(ch, rate, q):
    import vorbis_aotuv_lancer_amd as v
    return v.header_packets(v.Setup(ch, rate, q))


def matrix_classes():
    """(channels, rate, quality) of the shipped VBR packs that lie in the reference's test matrix (test/test.c:38-57)"""
    out = []
    for f in sorted(glob.glob(os.path.join(DATA, "mode_*ch_*_q*.vpk"))):
        m = re.match(r"mode_(\d+)ch_(\d+)_q(-?[\d.]+)\.vpk", os.path.basename(f))
        ch, rate, q = int(m.group(1)), int(m.group(2)), float(m.group(3))
        if 1 <= ch <= 8 and rate in (44100, 48000, 32000, 22050, 16000, 96000):
            out.append((ch, rate, q))
    return out


def oracle_packets(oracle, ch, rate, q, seconds=3.0, seed=3, bitrate=None, capture=True):
    """oracle encode of a burst signal (all four block types) -> list of block dicts, with the encode-side captures
    unless capture is off (then "packet" and the packet's own fields alone)"""
    return walk(oracle, ch, rate, None if bitrate else q, bitrate, burst_signal(ch, rate, int(seconds * rate), seed=seed),
                capture=capture)


def render_line(x0, x1, y0, y1, n):
    """floor1_inverse2's render_line (lib/floor1.c:368) as indices, bins [x0, min(n, x1))"""
    out = {}
    dy, adx = y1 - y0, x1 - x0
    base = int(dy / adx)
    sy = base - 1 if dy < 0 else base + 1
    ady = abs(dy) - abs(base) * adx
    x, y, err = x0, y0, 0
    if x < min(n, x1):
        out[x] = y
    x += 1
    while x < min(n, x1):
        err += ady
        if err >= adx:
            err -= adx
            y += sy
        else:
            y += base
        out[x] = y
        x += 1
    return out


def floor_expected(ref, enc_x1, mode, ilogmask, n):
    """The floor line a decoder renders, from the encoder's ilogmask capture.  Equal to the capture, except on a floor
    whose last post the encoder keeps at an x the header cannot express: floor1_pack writes rangebits = ilog(x1) and
    every decoder takes postlist[1] = 1 << rangebits (lib/floor1.c:119-182), so the 5.1 packs' LFE floor (posts
    {0, 12}, no interior post) is encoded over [0, 12) and decoded over [0, 16).  There the expected line is rendered
    from the capture's two end values over the header's range."""
    want = np.array(ilogmask, copy=True)
    m = ref["maps"][ref["modes"][mode][3]]
    for c in range(want.shape[0]):
        f = ref["floors"][m["floorsubmap"][m["chmuxlist"][c]]]
        hx = f["postlist"][1]
        ex = enc_x1[m["floorsubmap"][m["chmuxlist"][c]]]
        if hx == ex or not want[c].any():
            continue
        assert len(f["postlist"]) == 2, "only a floor without interior posts can be restated from its end values"
        y0, y1 = int(want[c, 0]), int(want[c, n - 1])
        for x, y in render_line(0, hx, y0, y1, n).items():
            want[c, x] = y
        want[c, min(hx, n):] = y1
    return want


def residue_coded(ref, mode, ch, n, nonzero):
    """mask [ch][n] of the bins the mode's residue setup codes (lib/res0.c:_01inverse / res2_inverse)"""
    m = ref["maps"][ref["modes"][mode][3]]
    mask = np.zeros((ch, n), bool)
    for sm in range(m["submaps"]):
        r = ref["residues"][m["residuesubmap"][sm]]
        chans = [c for c in range(ch) if m["chmuxlist"][c] == sm]
        if r["type"] == 2:
            if not any(nonzero[c] for c in chans):
                continue
            nb = len(chans)
            end = min(r["end"], n * nb)
            coded = (end - r["begin"]) // r["grouping"] * r["grouping"]
            for i, c in enumerate(chans):
                k = np.arange(n) * nb + i
                mask[c] = (k >= r["begin"]) & (k < r["begin"] + coded)
        else:
            end = min(r["end"], n)
            coded = (end - r["begin"]) // r["grouping"] * r["grouping"]
            for c in chans:
                if nonzero[c]:
                    mask[c, r["begin"]:r["begin"] + max(coded, 0)] = True
    return mask


# ---- the model's corpus --------------------------------------------------------------------------------------------
def fromdB():
    import vorbis_aotuv_lancer_amd as v
    return v.tables.pack("common.vpk")["FLOOR1_fromdB_LOOKUP"]


def unpack_differs(got, want):
    """host unpack (status, info, floor index, residue, used) against a model result -> what differs, or None"""
    rc, info, findex, res, used = got
    if rc != want["status"]:
        return f"status {rc}, model {want['status']}"
    if list(info) != want["info"]:
        return f"info {list(info)}, model {want['info']}"
    if not np.array_equal(used, want["used"]):
        return f"floor used {used}, model {want['used']}"
    if not np.array_equal(findex, want["floor_index"]):
        return f"floor index at {np.argwhere(findex != want['floor_index'])[:4].tolist()}"
    if res.tobytes() != want["residue"].tobytes():
        return f"residue at {np.argwhere(res != want['residue'])[:4].tolist()}"
    return None


@functools.lru_cache(maxsize=None)
def family(k):
    """vm.CORPUS[k] -> (setup dict, header coding, headers, model counters, [(label, packet, model result)], ds facts,
    the packets on which the host unpack differs from the model)"""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.build_corpus_setup(k)
    h = vm.pack_headers(setup, coding)
    assert v.DecodeSetup.status(h) == 0, v.lib.vbm_last_error()
    ds = v.DecodeSetup(h)
    facts = (ds.counts(), list(ds.blocksizes), ds.modes, ds.channels)
    model = vm.Model(setup, fromdB())
    rows, bad = [], []
    for label, p in vm.corpus_packets(model, h, 5000 + k):
        r = model.decode(p)
        vm.check_scales(r)
        diff = unpack_differs(ds.unpack(p), r)
        if diff:
            bad.append(f"{label}: {diff}")
        rows.append((label, p, r))
    ds.close()
    return setup, coding, h, dict(model.C), rows, facts, bad


def bad_mode_packet(modes, modebits):
    """an audio packet whose mode is one past the last: VBM_EBADPACKET"""
    w = vm.BitWriter()
    w.write(0, 1)
    w.write(modes, modebits)
    w.write(0xABCDE, 20)
    return w.tobytes()


def with_failed_packets(streams, headers, modes, modebits):
    """the streams with packets that fail inside them: a header packet, the empty packet, a mode past the last"""
    out = []
    for s, pk in enumerate(streams):
        pk = list(pk)
        pk.insert(3, (headers[2], -1, 0))
        pk.insert(6, (b"", -1, 0))
        if modes < (1 << modebits):
            pk.insert(2 + s, (bad_mode_packet(modes, modebits), -1, 0))
        out.append(pk)
    return out


# vm.pcm_setup numbers of the runs and ranges tests: one setup per residue type (the 256/256 one has bs0 = bs1), and a
# pair of equal large blocks
RUNS = [("pair_256_256_grouping1", 0), ("res0", 2), ("res2", 1), ("res1_3modes", 3), ("pair_1024_1024", 9)]


def random_stream_packets(k, seed):
    """a seeded random stream on block-size pair k: 40 packets whose W sequence has all four transitions (when the
    pair has two sizes), with failed packets inside -> (ds, packets)"""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(k)
    h = vm.pack_headers(setup, coding)
    ds = v.DecodeSetup(h)
    model = vm.Model(setup, fromdB())
    rng = np.random.default_rng(seed)
    seq = "SSLLS" + "".join(rng.choice(["S", "L"], 35))
    packets = [p for p, _, _ in vm.pcm_streams(model, seed, sequences=[seq])[0]]
    W = [ds.unpack(p)[1][1] for p in packets]
    if ds.blocksizes[0] != ds.blocksizes[1]:
        assert {(a, b) for a, b in zip(W, W[1:])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    modes, bits = len(setup["modes"]), model.modebits
    packets.insert(9, h[2])                                  # a header packet: VBM_ENOTAUDIO
    packets.insert(17, b"")                                  # the empty packet
    if modes < (1 << bits):
        packets.insert(23, bad_mode_packet(modes, bits))
    packets.insert(1, h[0])                                  # a failed packet before the second block
    return ds, packets


# ---- packet lists and their CSR forms ------------------------------------------------------------------------------
def split_dump(d):
    """a packet dump of tests/golden (per packet a 32-bit length, then the bytes) -> [packet]"""
    out, at = [], 0
    while at < len(d):
        n = int.from_bytes(d[at:at + 4], "little")
        out.append(d[at + 4:at + 4 + n])
        at += 4 + n
    return out


def dump_packets(name):
    return split_dump(open(os.path.join(G, name), "rb").read())


def csr(packets):
    """[packet] -> (data uint8, offsets int64 [P + 1])"""
    data = np.frombuffer(b"".join(packets), np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in packets]).astype(np.int64)
    return data, offs


def as_stream(rows):
    """[(packet, granulepos, eos)] -> (data, offsets, granulepos, eos) numpy, as demux_ogg returns a stream"""
    return (*csr([p[0] for p in rows]), np.array([p[1] for p in rows], np.int64),
            np.array([p[2] for p in rows], np.uint8))


def join(streams):
    """[(data, offsets, granulepos, eos)] -> one CSR (data, offsets, granulepos, eos, stream_packets)"""
    datas, offs, gps, eoss, first, base = [], [np.zeros(1, np.int64)], [], [], [0], 0
    for data, o, gp, eo in streams:
        datas.append(np.asarray(data, np.uint8))
        offs.append(np.asarray(o[1:], np.int64) + base)
        gps.append(np.asarray(gp, np.int64))
        eoss.append(np.asarray(eo, np.uint8))
        first.append(first[-1] + len(o) - 1)
        base += len(data)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)      # noqa: E731
    return (cat(datas, np.uint8), cat(offs, np.int64), cat(gps, np.int64), cat(eoss, np.uint8),
            np.asarray(first, np.int64))


def ogg_packets(blob):
    """an .ogg file -> (headers, [(packet, granulepos, eos)])"""
    import vorbis_aotuv_lancer_amd as v
    headers, data, offsets, gp, eos = v.demux_ogg(blob)
    data = np.asarray(data, np.uint8).tobytes()
    return headers, [(data[int(a):int(b)], int(g), int(e)) for a, b, g, e in zip(offsets[:-1], offsets[1:], gp, eos)]


def with_bad_packets(packets, headers, seed):
    rng = np.random.default_rng(seed)
    bad = list(packets)
    bad.insert(min(10, len(bad)), headers[2])
    bad.insert(min(20, len(bad)), packets[min(19, len(packets) - 1)][:len(packets[min(19, len(packets) - 1)]) // 3])
    bad.insert(min(30, len(bad)), rng.integers(0, 256, 200, dtype=np.uint8).tobytes())
    bad.insert(min(31, len(bad)), b"")
    bad.insert(0, headers[0])
    bad.insert(1, b"\x00")                               # a one-byte audio packet: the mode is missing
    return bad


def serial_index(v, ds, data, offsets, gp, eos, first, halfrate):
    """vbm_decode_index_halfrate of every stream alone -> (status, samples, out_start, totals) over the whole CSR"""
    st, sm, os_, tot = [], [], [], []
    for a, b in zip(first[:-1], first[1:]):
        r = v.decode_index(ds, data, offsets[a:b + 1], None if gp is None else gp[a:b],
                           None if eos is None else eos[a:b], halfrate=halfrate)
        st.append(r[0]), sm.append(r[1]), os_.append(r[2]), tot.append(r[3])
    return (np.concatenate(st), np.concatenate(sm), np.concatenate(os_), np.asarray(tot, np.int64))


# ---- seeded streams of one-byte packets (Setup(2, 44100, 0.5): modebits 1, mode 0 short, mode 1 long) ----------------
BS = (256, 2048)
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 4097]
GP_KINDS = ["none", "jitter", "jitter0", "zero", "big", "minus2", "minus129", "land"]


def one_byte_stream(rng, n, invalid, kind, last_eos, first_valid=0):
    """n packets of one byte: bit 0 the packet type (1: not audio), bit 1 the mode, bits 2 and 3 lW and nW
    -> (data, offsets, granulepos, eos)"""
    bad = rng.random(n) < invalid
    bad[:first_valid] = True
    mode = rng.integers(0, 2, n)
    data = (bad.astype(np.uint8) | (mode << 1) | (rng.integers(0, 4, n) << 2)).astype(np.uint8)
    # the count an encoder would write (sum of the steps), and the step of every valid packet
    count, step, lW, g = np.zeros(n, np.int64), np.zeros(n, np.int64), -1, 0
    for k in range(n):
        if not bad[k]:
            step[k] = (BS[lW] // 4 if lW >= 0 else 0) + BS[mode[k]] // 4
            if lW >= 0:
                g += step[k]
            lW = mode[k]
        count[k] = g
    gp = np.full(n, -1, np.int64)
    some = rng.random(n) < 0.2
    if kind in ("jitter", "jitter0"):
        gp[some] = (count + rng.integers(-3000, 3001, n))[some]
        if kind == "jitter0":
            gp[some] = np.maximum(gp[some], 0)
    elif kind == "zero":
        gp[some] = np.where(rng.random(n) < 0.5, 0, count)[some]
    elif kind == "big":
        gp[some] = np.where(rng.random(n) < 0.5, 2 ** 40, count)[some]
    elif kind in ("minus2", "minus129"):
        gp[some] = np.where(rng.random(n) < 0.5, -2 if kind == "minus2" else -129, count)[some]
    elif kind == "land":
        # -1 - (the next valid packet's step): the running position lands on -1 there and is "none yet" again
        nxt = np.full(n, 128, np.int64)
        valid = np.flatnonzero(~bad)
        for a, b in zip(valid[:-1], valid[1:]):
            nxt[a] = BS[mode[a]] // 4 + BS[mode[b]] // 4
        gp[some] = np.where(rng.random(n) < 0.5, -1 - nxt, count)[some]
    eos = (rng.random(n) < 0.1).astype(np.uint8)
    if n:
        eos[-1] = last_eos
    return data, np.arange(n + 1, dtype=np.int64), gp, eos


def one_byte_corpus(seed=1, lengths=LENGTHS, kinds=GP_KINDS, shares=(0.0, 0.1, 0.9)):
    rng = np.random.default_rng(seed)
    streams = []
    for n in lengths:
        for invalid in shares:
            for kind in kinds:
                streams.append(one_byte_stream(rng, n, invalid, kind, int(rng.integers(0, 2))))
    for kind in kinds:
        streams.append(one_byte_stream(rng, 150, 1.0, kind, 1))                    # no valid packet at all
        streams.append(one_byte_stream(rng, 150, 0.1, kind, 1, first_valid=64))    # the first valid packet is 64
    return streams


# ---- the reference's blockin bookkeeping, once ---------------------------------------------------------------------
def blockin(bs, hs, status, W, granulepos, eos, gap=None, lW=-1):
    """vorbis_synthesis_blockin's sample bookkeeping (lib/block.c:907-915 and 1050-1161) for one stream from its start.
    Per packet: status (non-zero: the packet failed and reaches blockin not at all), the block flag W (read only where
    the status is 0), the granule position (-1: none), the end flag and, optionally, a gap mark (packets were lost in
    front of this one).  bs: the two block sizes; hs: ci->halfrate_flag; lW: the block flag of the packet before the
    first (-1: a fresh stream).  pcm_returned and pcm_current are taken relative to the packet's first final sample.
    -> (samples returned per packet, out_start per packet, the stream's total)"""
    sample_count, pos, at, lost = -1, -1, 0, False
    samples, out_start = [], []
    for k, rc in enumerate(status):
        out_start.append(at)
        lost = lost or bool(gap is not None and gap[k])      # a mark on a failed packet waits for the next valid one
        if rc:
            samples.append(0)
            continue
        if lost:                                             # :911-915: out of sequence, the stream loses count
            sample_count = pos = -1
            lost = False
        step = (bs[lW] // 4 if lW >= 0 else 0) + bs[W[k]] // 4
        pcm_returned = 0                                     # :1059-1062 (a first block: both at thisCenter)
        pcm_current = step >> hs if lW >= 0 else 0
        sample_count = 0 if sample_count == -1 else sample_count + step      # :1078-1082
        if pos == -1:                                        # :1084-1125
            if granulepos[k] != -1:
                pos = granulepos[k]
                if sample_count > pos:
                    extra = max(sample_count - granulepos[k], 0)
                    if eos[k]:
                        # edge 1: extra is clamped with << hs and applied with >> hs (:1102-1115)
                        extra = min(extra, (pcm_current - pcm_returned) << hs)
                        pcm_current -= extra >> hs
                    else:
                        # edge 2: after a start trim, pcm_returned is clamped to pcm_current (:1117-1121)
                        pcm_returned = min(pcm_returned + (extra >> hs), pcm_current)
        else:                                                # :1126-1157
            pos += step
            if granulepos[k] != -1 and pos != granulepos[k]:
                if pos > granulepos[k] and eos[k]:
                    extra = max(min(pos - granulepos[k], (pcm_current - pcm_returned) << hs), 0)     # edge 1 again
                    pcm_current -= extra >> hs
                pos = granulepos[k]
        n = pcm_current - pcm_returned                       # vorbis_synthesis_pcmout + _read
        samples.append(n)
        at += n
        lW = W[k]
    return samples, out_start, at


def restated(ds, packets, gps, eoss, hs=0):
    """`blockin` over the host unpack's status and W -> (status, samples, out_start, total)"""
    heads = [ds.unpack(p)[:2] for p in packets]
    status = [rc for rc, _ in heads]
    W = [0 if rc else info[1] for rc, info in heads]
    return (status, *blockin(ds.blocksizes, hs, status, W, gps, eoss))


def true_granules(ds, packets):
    """the granule position an encoder writes after each packet, in full-rate samples: the sum of the blockin steps
    (failed packets repeat the last)"""
    bs, lW, g, out = ds.blocksizes, -1, 0, []
    for p in packets:
        rc, info = ds.unpack(p)[:2]
        if rc == 0:
            if lW >= 0:
                g += bs[lW] // 4 + bs[info[1]] // 4
            lW = info[1]
        out.append(g)
    return out


def page_granule_variants(ds, packets):
    """(granulepos, eos) lists: none; on every 7th packet and the last with eos; a lowered first granulepos
    (trimmed start); an eos trim of 300 samples"""
    n, g = len(packets), true_granules(ds, packets)
    none = ([-1] * n, [0] * n)
    pages = ([g[k] if (k % 7 == 6 or k == n - 1) else -1 for k in range(n)], [0] * (n - 1) + [1])
    low = list(pages[0])
    first = next(k for k in range(n) if low[k] != -1)
    low[first] = max(low[first] - 700, 0)
    trim = list(pages[0])
    trim[-1] = max(trim[-1] - 300, 0)
    return [none, pages, (low, pages[1]), (trim, pages[1])]


def trim_granule_variants(ds, packets):
    """(name, granulepos, eos): absent; exact; the last packet short by odd and even amounts (end trim), with and
    without earlier positions; the first marked packet short by odd and even amounts (start trim), and by more than
    it returns; the last packet backdated by more than the stream holds (the clamp), with and without earlier
    positions; a start trim on the stream's first packet"""
    n, g = len(packets), true_granules(ds, packets)
    valid = [k for k in range(n) if ds.unpack(packets[k])[0] == 0]
    assert valid[-1] == n - 1
    eos = [0] * (n - 1) + [1]
    exact = [g[k] if (k in valid and (k % 5 == 4 or k == n - 1)) else -1 for k in range(n)]
    first = next(k for k in range(n) if exact[k] != -1)
    out = [("absent", [-1] * n, [0] * n), ("exact", exact, eos)]
    for d in (1, 2, 37, 300, 301):
        a = list(exact)
        a[-1] = g[-1] - d
        out.append((f"end trim {d}", a, eos))
        b = [-1] * (n - 1) + [g[-1] - d]                     # the first marked packet is the last: lib/block.c:1102
        out.append((f"end trim {d}, no earlier position", b, eos))
        c = list(exact)
        c[first] = g[first] - d
        out.append((f"start trim {d}", c, eos))
    c = list(exact)
    c[first] = max(g[first] - 3 * ds.blocksizes[1], 0)
    out.append(("start trim past the packet", c, eos))
    a = list(exact)
    a[-1] = 0
    out.append(("backdated last packet", a, eos))
    out.append(("backdated last packet, no earlier position", [-1] * (n - 1) + [0], eos))
    odd = list(exact)
    odd[-1] = 1
    out.append(("backdated to 1", odd, eos))
    z = list(exact)
    z[0] = 0                                                 # sample_count 0 is not past 0: nothing trimmed
    out.append(("position on the first packet", z, eos))
    return out
