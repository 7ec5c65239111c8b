"""Decoder, host side (no GPU): header parse against the shipped packs and an independent Python unpacker, the
reference's error codes for malformed headers, exact parity of the packet unpack with the oracle's encode-side
captures, truncated packets, and Ogg read-back."""
import glob
import os

import numpy as np
import pytest

from tests import orc
from tests.signals import burst_signal
from tests.test_stream_wrapper import unpack_headers
import vpk  # noqa: E402  (tools/, on the path once test_stream_wrapper is imported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "vorbis_aotuv_lancer_amd", "data")

ENOTVORBIS, EBADHEADER, EVERSION, ENOTAUDIO, EBADPACKET, EIMPL, ENODEV = -132, -133, -134, -135, -136, -130, -1000

# (channels, rate, quality): the classes of the unpack parity test
PARITY = [(2, 44100, 0.5), (2, 44100, 0.1), (6, 48000, 0.8), (1, 44100, 0.5), (8, 44100, 0.5), (2, 96000, 0.5)]


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


def oracle_packets(oracle, ch, rate, q, seconds=3.0, seed=3):
    """oracle encode with capture of a burst signal (all four block types) -> list of block dicts"""
    st = orc.Stream(orc.Setup(oracle, ch, rate, q))
    sig = burst_signal(ch, rate, int(seconds * rate), seed=seed)
    blocks = []
    for i in range(0, sig.shape[1], 1024):
        st.write(sig[:, i:i + 1024])
        blocks.extend(st.blocks())
    st.finish()
    blocks.extend(st.blocks())
    st.close()
    return blocks


@pytest.mark.parametrize("pack", sorted(os.path.basename(p) for p in glob.glob(os.path.join(DATA, "mode_*.vpk"))))
def test_header_parse_matches_the_pack_and_the_python_unpacker(pack):
    import vorbis_aotuv_lancer_amd as v
    setup, d = pack_setup(v, pack)
    h = v.header_packets(setup)
    ds = v.DecodeSetup(h)
    assert ds.channels == int(d["info/channels"][0]) and ds.rate == int(d["info/rate"][0])
    ref = unpack_headers(*h)
    assert list(ds.blocksizes) == ref["blocksizes"] and ds.modes == len(ref["modes"])
    assert ds.counts() == (len(ref["books"]), len(ref["floors"]), len(ref["residues"]), len(ref["maps"]))
    ds.close()


class _Bits:
    """bit positions of the fields the malformed-header tests edit (LSb-first packing)"""

    def __init__(self, data):
        self.d, self.pos = bytes(data), 0

    def read(self, n):
        v = 0
        for i in range(n):
            v |= ((self.d[(self.pos + i) >> 3] >> ((self.pos + i) & 7)) & 1) << i
        self.pos += n
        return v


def set_bits(data, pos, n, value):
    b = bytearray(data)
    for i in range(n):
        byte, bit = (pos + i) >> 3, (pos + i) & 7
        b[byte] = (b[byte] & ~(1 << bit)) | (((value >> i) & 1) << bit)
    return bytes(b)


def floor_type_bit(h2):
    """bit position of the first floor type field of a setup header (after the books and time placeholders)"""
    from tests.test_stream_wrapper import BitReader, unpack_book
    r = BitReader(h2)
    for _ in range(7):
        r.read(8)
    for _ in range(r.read(8) + 1):
        unpack_book(r)
    for _ in range(r.read(6) + 1):
        r.read(16)
    r.read(6)
    return r.pos


def test_malformed_headers_return_the_reference_codes():
    import vorbis_aotuv_lancer_amd as v
    h0, h1, h2 = headers_of(2, 44100, 0.5)
    S = v.DecodeSetup.status
    assert S([h0, h1, h2]) == 0
    assert S([b"\x01xorbis" + h0[7:], h1, h2]) == ENOTVORBIS              # signature
    assert S([h0, h1, b"\x05vorbiz" + h2[7:]]) == ENOTVORBIS
    assert S([h1, h0, h2]) == EBADHEADER                                   # out of order
    assert S([h0, h2, h1]) == EBADHEADER
    assert S([h0[:-1] + bytes([h0[-1] & 0xFE]), h1, h2]) == EBADHEADER    # framing bit of the identification header
    assert S([h0, h1[:-1] + bytes([0]), h2]) == EBADHEADER                # framing bit of the comment header
    assert S([h0[:7] + b"\x01" + h0[8:], h1, h2]) == EVERSION              # version 1
    # block-size nibbles: byte 28 = blocksize_0 (low nibble), blocksize_1 (high nibble)
    assert S([h0[:28] + bytes([(h0[28] & 0x0F) | (13 << 4)]) + h0[29:], h1, h2]) == EIMPL   # 8192
    # floor type 0
    pos = floor_type_bit(h2)
    assert _Bits(h2[pos >> 3:]).read(8 + (pos & 7)) >> (pos & 7) == 1
    assert S([h0, h1, set_bits(h2, pos, 16, 0)]) == EIMPL
    # a setup header cut short
    assert S([h0, h1, h2[:len(h2) // 2]]) == EBADHEADER


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


@pytest.mark.parametrize("ch,rate,q", PARITY)
def test_unpack_matches_the_oracle_captures_exactly(oracle, ch, rate, q):
    import vorbis_aotuv_lancer_amd as v
    h = headers_of(ch, rate, q)
    ref = unpack_headers(*h)
    ds = v.DecodeSetup(h)
    blocks = oracle_packets(oracle, ch, rate, q)
    pack = vpk.read_vpk(os.path.join(DATA, orc.mode_pack_name(ch, rate, q)))
    enc_x1 = [int(pack[f"floor/{i}/postlist"][1]) for i in range(len(ref["floors"]))]
    kinds = set()
    for k, b in enumerate(blocks):
        rc, info, findex, res, used = ds.unpack(b["packet"])
        assert rc == 0, f"packet {k}"
        W = info[1]
        n = ds.blocksizes[W] // 2
        assert W == b["W"], f"packet {k}"
        if W:
            assert (info[2], info[3]) == (b["lW"], b["nW"]), f"packet {k}"
        kinds.add((b["lW"], b["W"], b["nW"]) if W else (0, 0, 0))
        assert list(used) == list(b["nonzero"]), f"packet {k}: floor-used flags"
        # the floor line as indices: the encoder's ilogmask (floor1_encode renders the same line; 0 where the
        # channel's floor is not coded)
        np.testing.assert_array_equal(findex[:, :n], floor_expected(ref, enc_x1, info[0], b["ilogmask"], n),
                                      err_msg=f"packet {k}: floor index")
        assert not findex[:, n:].any()
        # residue: the quantised values over the bins the residue setup codes.  The encoder quantises every bin of
        # the block, but res0/1/2 code only [begin, begin + partitions*grouping) of the (interleaved, residue 2)
        # vector, so the values above that range are never sent.
        mask = residue_coded(ref, info[0], ch, n, b["nonzero"])
        want = np.where(mask, b["residue"].astype(np.float32), np.float32(0))
        np.testing.assert_array_equal(res[:, :n], want, err_msg=f"packet {k}: residue")
        assert not res[:, n:].any()
    if ds.blocksizes[0] != ds.blocksizes[1]:
        assert {(0, 0, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)} <= kinds, kinds   # short, and long after / before short
    ds.close()


def test_truncated_packets_decode_without_fault_and_with_the_reference_status(oracle):
    import vorbis_aotuv_lancer_amd as v
    h = headers_of(2, 44100, 0.5)
    ds = v.DecodeSetup(h)
    blocks = oracle_packets(oracle, 2, 44100, 0.5, seconds=1.5)
    assert ds.unpack(b"")[0] == ENOTAUDIO
    for b in blocks:
        full = b["packet"]
        _, info_full, _, _, _ = ds.unpack(full)
        for cut in range(len(full) + 1):
            rc, info, findex, res, used = ds.unpack(full[:cut])
            if cut == 0:
                assert rc == ENOTAUDIO
                continue
            # one bit of packet type and one of mode (2 modes): a single byte always has both
            assert rc == 0
            assert info[:2] == info_full[:2]
            assert np.isfinite(res).all() and (findex >= 0).all() and (findex < 256).all()
    # a header packet is not audio
    for hp in h:
        assert ds.unpack(hp)[0] == ENOTAUDIO
    ds.close()


def test_bad_mode_is_ebadpacket():
    import vorbis_aotuv_lancer_amd as v
    ds = v.DecodeSetup(headers_of(2, 44100, 0.5))          # 2 modes: 1 mode bit
    assert ds.modes == 2
    ds1 = v.DecodeSetup(headers_of(2, 44100, 0.5))
    # long block (mode 1) packet of a single byte: W=1 needs lW and nW bits -> those fit in the byte
    assert ds1.unpack(bytes([0b00000010]))[0] == 0
    ds.close()
    ds1.close()


def test_read_ogg_inverts_write_ogg(oracle):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    blocks = oracle_packets(oracle, 2, 44100, 0.5, seconds=2.0)
    packets = [b["packet"] for b in blocks]
    infos = [(b["granulepos"], bool(b["eos"])) for b in blocks]
    assert infos[-1][1]
    data = v.write_ogg(setup, packets, infos)
    headers, got, gps, eos = v.read_ogg(data)
    assert headers == v.header_packets(setup)
    assert got == packets
    # the granule position travels per page: the last packet that ends on a page carries it, the others read -1
    # (libogg's ogg_stream_packetout); eos is the last packet's
    assert gps[-1] == infos[-1][0] and eos[-1] and not any(eos[:-1])
    carried = [i for i, g in enumerate(gps) if g != -1]
    assert carried and all(gps[i] == infos[i][0] for i in carried)
    bad = bytearray(data)
    bad[len(bad) // 2] ^= 0x40
    with pytest.raises(ValueError):
        v.read_ogg(bytes(bad))


def test_decoder_create_without_a_device_is_enodev():
    """in a child process that sees no HIP device (on a GPU machine too)"""
    import subprocess
    import sys
    code = (
        "import ctypes as C, sys\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import vorbis_aotuv_lancer_amd as v\n"
        "ds = v.DecodeSetup(v.header_packets(v.Setup(2, 44100, 0.5)))\n"
        "h = C.c_void_p()\n"
        "print(v.lib.vbm_decoder_create(C.byref(h), ds._h, 4, 4))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == ENODEV
