"""Shared by test_ogg_demux_batch_cpu.py and test_ogg_demux_gpu.py: the file corpora of the batch Ogg demux, the C calls of
its host twin and of the device form over one interface, and the single-file yardstick (vbm_ogg_demux)."""
import ctypes as C
import functools

import numpy as np

from tests.ogg_pages import corruptions, pack, random_bytes, split_pages
from tests.ogg_twin import Result, Twin, lib as _lib

EOGG, EINVAL, ECAP = -1002, -131, 1


def _info_dtype():
    from vorbis_aotuv_lancer_amd.stream import FILE_INFO
    return FILE_INFO


# ---- corpora -----------------------------------------------------------------------------------------------------------

def _paged(v, packets, flush_after_headers, comments=(), setup=None):
    """headers + (packet, granulepos) through OggStream; without the flush the setup header shares its page with audio"""
    setup = setup or v.Setup(1, 44100, 0.1)
    os_ = v.OggStream(77)
    out = []
    for h in v.header_packets(setup, comments):
        os_.packetin(h, 0)
        out += os_.pages()                       # the first page goes out alone; nothing else is due yet
    if flush_after_headers:
        out += os_.pages(flush=True)
    for k, p in enumerate(packets):
        os_.packetin(p, 100 * (k + 1), k == len(packets) - 1)
        out += os_.pages()
    out += os_.pages(flush=True)
    os_.close()
    return b"".join(out)


def streams(v):
    """(name, .ogg bytes) of write_ogg output: several classes' headers, with packets that span pages, packets whose
    lengths are multiples of 255 (0 included), and an eos packet"""
    rng = np.random.default_rng(5)
    out = []
    for ch, rate, q in [(1, 44100, 0.1), (2, 44100, 0.5), (6, 48000, 0.8), (2, 96000, 0.5)]:
        setup = v.Setup(ch, rate, q)
        lens = [1, 254, 255, 256, 510, 0, 765, 4097, 70000, 255 * 255, 255 * 255 + 1, 3, 255 * 3, 2, 300] * 2
        pk = [random_bytes(rng, n) for n in lens]
        infos = [(-1 if k % 3 == 1 else 1024 * (k + 1), k == len(pk) - 1) for k in range(len(pk))]
        out.append((f"{ch}ch_{rate}_q{q}", v.write_ogg(setup, pk, infos, serialno=0x1234 + ch)))
    # many small packets: pages that close on the 4096-byte / 4-packet rule and on 255 segments
    setup = v.Setup(2, 44100, 0.5)
    pk = [random_bytes(rng, n) for n in rng.integers(0, 600, 700)]
    out.append(("small_packets", v.write_ogg(setup, pk, [(k * 512, k == len(pk) - 1) for k in range(len(pk))])))
    return out


@functools.lru_cache(maxsize=None)
def directed():
    """(name, blob): the shapes the issue lists, valid files, but for the last"""
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(21)
    rb = functools.partial(random_bytes, rng)
    out = [("zero length", b""),
           ("headers alone", v.write_ogg(v.Setup(2, 44100, 0.5), [], []))]
    # 240 one-byte packets then 70000 bytes: 15 + 255 + 5 segments of it on three pages, the middle one of 255 segments
    out.append(("packet over three pages", _paged(v, [rb(1) for _ in range(240)] + [rb(70000), rb(9)], True)))
    out.append(("multiples of 255", _paged(v, [rb(n) for n in (255, 0, 510, 255 * 255, 0, 0, 765, 255)], True)))
    # no flush after the headers: comment and setup header share the second page with the first audio packets
    out.append(("setup header shares its page", _paged(v, [rb(n) for n in (30, 300, 5, 700, 2)], False)))
    # a comment header of 70 KB: a header packet over several pages, and then the setup header and audio on one page
    out.append(("header packet spans pages", _paged(v, [rb(n) for n in (40, 41, 600)], False, comments=["k=" + "x" * 70000])))
    # the same without its last two pages: the 70000-byte packet is open at the end of the data and is dropped
    out.append(("unterminated packet at the end", b"".join(split_pages(out[2][1], as_bytes=True)[:-2])))
    out.append(("truncated", out[3][1][:-200]))                                                   # VBM_EOGG
    return out


@functools.lru_cache(maxsize=None)
def mixed():
    """the five streams files and every corruptions variant of the second, good and bad interleaved"""
    import vorbis_aotuv_lancer_amd as v
    good = streams(v)
    bad = list(corruptions(good[1][1]).items())
    out = []
    for k in range(max(len(good), len(bad))):
        if k < len(bad):
            out.append(bad[k])
        if k < len(good):
            out.append(good[k])
    return out


@functools.lru_cache(maxsize=None)
def six_packet_file():
    """the file of test_demux_never_reads_past_n and the ends of its pages"""
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(9)
    pk = [random_bytes(rng, n) for n in (300, 255, 1, 600, 0, 2000)]
    blob = v.write_ogg(v.Setup(1, 44100, 0.1), pk, [(100 * k, k == len(pk) - 1) for k in range(len(pk))])
    bounds, pos = set(), 0
    for p in split_pages(blob):
        pos += len(p)
        bounds.add(pos)
    return blob, bounds


# ---- the yardstick -----------------------------------------------------------------------------------------------------

def single(blob):
    """vbm_ogg_demux on one file -> None for VBM_EOGG, else (header_bytes [3], headers, payload, offsets, granulepos,
    eos) as bytes / numpy"""
    lib = _lib()
    buf = (C.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
    sizes = (C.c_long * 5)()
    rc = lib.vbm_ogg_demux(buf, len(blob), sizes, None, None, None, None, None)
    if rc == EOGG:
        return None
    assert rc == 0, rc
    hdr = np.zeros(sizes[0] + sizes[1] + sizes[2], np.uint8)
    body, offs = np.zeros(sizes[4], np.uint8), np.zeros(sizes[3] + 1, np.int64)
    gp, eos = np.zeros(sizes[3], np.int64), np.zeros(sizes[3], np.uint8)
    assert lib.vbm_ogg_demux(buf, len(blob), sizes, hdr.ctypes.data, body.ctypes.data, offs.ctypes.data, gp.ctypes.data,
                             eos.ctypes.data) == 0
    return list(sizes[:3]), hdr.tobytes(), body.tobytes(), offs, gp, eos


# ---- the host twin and the device calls (ogg_twin.Twin) ------------------------------------------------------------------

class Batch(Twin):
    """A demuxer and its buffers"""

    def __init__(self, impl, max_files, max_bytes):
        super().__init__(impl, "demuxer", max_files, max_bytes, status_name="demux_status")

    def scan_raw(self, nfiles, data_ptr, off_ptr, info_ptr, totals_ptr):
        return self.call("demux_scan", nfiles, data_ptr, off_ptr, info_ptr, totals_ptr)

    def fill_raw(self, hdr, hcap, pay, pcap, offs, gp, eos, kcap):
        return self.call("demux_fill", hdr, hcap, pay, pcap, offs, gp, eos, kcap)

    def scan(self, data, offsets):
        """data: uint8 numpy (or an address), offsets: int64 numpy [n + 1] -> (info, totals) as numpy"""
        n = len(offsets) - 1
        if isinstance(data, np.ndarray):
            data = self.upload(data)
        info = self.new(n * _info_dtype().itemsize, np.uint8)
        totals = self.new(3, np.int64, -1)
        off = np.ascontiguousarray(offsets, np.int64)
        rc = self.scan_raw(n, data, off.ctypes.data, self.ptr(info), self.ptr(totals))
        assert rc == 0, (rc, self.lib.vbm_last_error())
        return self.back(info).view(_info_dtype()), self.back(totals)

    def fill(self, totals, short=None, canary=8):
        """buffers of exactly the totals' sizes (short: 'packets' / 'payload' / 'headers' tells fill one less), `canary`
        blank elements behind each -> Result of numpy arrays without the canaries, .status, .touched (any buffer
        differs from its blank pattern), .canaries_ok"""
        P, B, H = (int(x) for x in totals)
        sizes = {"headers": (H, np.uint8), "payload": (B, np.uint8), "offsets": (P + 1, np.int64),
                 "granulepos": (P, np.int64), "eos": (P, np.uint8)}
        bufs = {name: self.guarded(n, dtype, canary) for name, (n, dtype) in sizes.items()}
        caps = {"packets": P, "payload": B, "headers": H}
        if short:
            caps[short] -= 1
        rc = self.fill_raw(self.ptr(bufs["headers"]), caps["headers"], self.ptr(bufs["payload"]), caps["payload"],
                           self.ptr(bufs["offsets"]), self.ptr(bufs["granulepos"]), self.ptr(bufs["eos"]), caps["packets"])
        assert rc == 0, (rc, self.lib.vbm_last_error())
        r = Result()
        r.status = self.status()
        r.touched, r.canaries_ok = False, True
        for name, buf in bufs.items():
            a, touched, ok = self.unguard(buf, sizes[name][0])
            r.touched, r.canaries_ok = r.touched or touched, r.canaries_ok and ok
            setattr(r, name, a)
        return r


def run(impl, blobs, first=0):
    """scan + fill of one batch whose first file starts at byte `first` of the buffer -> (info, totals, Result)"""
    data, offsets = pack(blobs, first)
    b = Batch(impl, max(1, len(blobs)), int(offsets[-1] - offsets[0]))
    try:
        info, totals = b.scan(data, offsets)
        return info, totals, b.fill(totals)
    finally:
        b.close()


def file_view(info, res, f):
    """file f of a batch -> what single() returns for it, or None"""
    fi = info[f]
    if fi["status"]:
        assert fi["status"] == EOGG
        return None
    hb, H = [int(x) for x in fi["header_bytes"]], int(fi["header_base"])
    a, n, at, nb = int(fi["packet_base"]), int(fi["packets"]), int(fi["payload_base"]), int(fi["payload_bytes"])
    return (hb, res.headers[H:H + sum(hb)].tobytes(), res.payload[at:at + nb].tobytes(), res.offsets[a:a + n + 1] - at,
            res.granulepos[a:a + n], res.eos[a:a + n])


def same(got, want):
    if got is None or want is None:
        return got is None and want is None
    return (got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and np.array_equal(got[3], want[3])
            and np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5]))


def check_csr(info, totals, res):
    """the properties of the batch's one CSR"""
    P, B, H = (int(x) for x in totals)
    assert res.offsets[0] == 0 and res.offsets[P] == B and (np.diff(res.offsets) >= 0).all()
    packets = payload = header = 0
    for fi in info:
        assert (fi["packet_base"], fi["payload_base"], fi["header_base"]) == (packets, payload, header)
        if fi["status"]:
            assert fi["status"] == EOGG
            assert (fi["pages"], fi["serialno"], fi["packets"], fi["payload_bytes"]) == (0, 0, 0, 0)
            assert not fi["header_bytes"].any()
        assert res.offsets[packets] == payload
        assert res.offsets[packets + fi["packets"]] == payload + fi["payload_bytes"]
        packets += int(fi["packets"])
        payload += int(fi["payload_bytes"])
        header += int(fi["header_bytes"].sum())
    assert (packets, payload, header) == (P, B, H)
