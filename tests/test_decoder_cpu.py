"""Decoder, host side (no GPU): header parse against the shipped packs and an independent Python unpacker, the
reference's error codes for malformed headers, exact parity of the packet unpack with the oracle's encode-side
captures, truncated packets, and Ogg read-back."""
import os

import numpy as np
import pytest

from tests import orc
from tests.decode_packets import (DATA, EBADHEADER, EIMPL, ENODEV, ENOTAUDIO, ENOTVORBIS, EVERSION, PACKS, PARITY,
                                  ROOT, BitReader, floor_expected, headers_of, oracle_packets, pack_setup,
                                  residue_coded, unpack_book, unpack_headers, vpk)


@pytest.mark.parametrize("pack", PACKS)
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


def set_bits(data, pos, n, value):
    b = bytearray(data)
    for i in range(n):
        byte, bit = (pos + i) >> 3, (pos + i) & 7
        b[byte] = (b[byte] & ~(1 << bit)) | (((value >> i) & 1) << bit)
    return bytes(b)


def floor_type_bit(h2):
    """bit position of the first floor type field of a setup header (after the books and time placeholders)"""
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
    assert BitReader(h2[pos >> 3:]).read(8 + (pos & 7)) >> (pos & 7) == 1
    assert S([h0, h1, set_bits(h2, pos, 16, 0)]) == EIMPL
    # a setup header cut short
    assert S([h0, h1, h2[:len(h2) // 2]]) == EBADHEADER


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
