"""Stream wrapper (host only — runs without a GPU).

Header packets: the product packs them like the reference's ENCODE side (vorbis_analysis_headerout).  The
check reads them back with a restatement of the reference's DECODE side (unpack_headers in tests/decode_packets.py)
— _vorbis_unpack_info/_comment/_books (lib/info.c:203-430), vorbis_staticbook_unpack (lib/codebook.c:277-395),
floor1_unpack (lib/floor1.c:119-180), res0_unpack (lib/res0.c:191-249), mapping0_unpack (lib/mapping0.c:95-160),
including their validity checks — and compares every field with the mode pack.  No reference header bytes exist to compare with
(parity with the reference unpinned); pack and unpack are different code in the reference, so the round
trip is an independent check.

Ogg pages: parsed back per the reference's doc/framing.html with an independent CRC (bitwise, no table), both in
tests/ogg_pages.py."""
import os

import numpy as np
import pytest

from tests.decode_packets import PACKS, ilog, pack_setup, unpack_headers
from tests.ogg_pages import crc_bitwise, packets_of, page_crc, parse_pages, split_pages


@pytest.mark.parametrize("pack", PACKS)
def test_header_packets_read_back_to_the_mode_pack(pack):
    import vorbis_aotuv_lancer_amd as v
    setup, d = pack_setup(v, pack)
    ch, rate = int(d["info/channels"][0]), int(d["info/rate"][0])
    comments = ["TITLE=parity", "ARTIST=" + "x" * 300]
    hdr = v.header_packets(setup, comments)
    u = unpack_headers(*hdr)
    assert (u["channels"], u["rate"]) == (ch, rate)
    assert u["blocksizes"] == [int(x) for x in d["info/blocksizes"]]
    assert u["bitrates"] == [int(x) & 0xffffffff for x in d["info/bitrates"]]
    assert u["vendor"] == b"AO; aoTuV [20110424] (based on libvorbis 1.3.7)"
    assert u["comments"] == [c.encode() for c in comments]
    modes_, maps_, floors_, residues_, books_, _ = [int(x) for x in d["info/counts"]]
    assert (len(u["modes"]), len(u["maps"]), len(u["floors"]), len(u["residues"]), len(u["books"])) == \
        (modes_, maps_, floors_, residues_, books_)
    for i, b in enumerate(u["books"]):
        head = [int(x) for x in d[f"book/{i}/head"]]
        assert (b["dim"], b["entries"], b["maptype"]) == (head[0], head[1], head[2])
        assert b["lengthlist"] == [int(x) for x in d[f"book/{i}/lengthlist"]]
        if b["maptype"]:
            assert (b["q_min"], b["q_delta"], b["q_quant"], b["q_sequencep"]) == \
                (head[3] & 0xffffffff, head[4] & 0xffffffff, head[5], head[6])
            assert b["quantlist"] == [abs(int(x)) for x in d[f"book/{i}/quantlist"]][:len(b["quantlist"])]
    for i, f in enumerate(u["floors"]):
        P = int(d[f"floor/{i}/partitions"][0])
        assert f["partitions"] == P and f["mult"] == int(d[f"floor/{i}/mult"][0])
        assert f["partitionclass"] == [int(x) for x in d[f"floor/{i}/partitionclass"][:P]]
        nc = len(f["class_dim"])
        assert f["class_dim"] == [int(x) for x in d[f"floor/{i}/class_dim"][:nc]]
        assert f["class_subs"] == [int(x) for x in d[f"floor/{i}/class_subs"][:nc]]
        for c in range(nc):
            if f["class_subs"][c]:
                assert f["class_book"][c] == int(d[f"floor/{i}/class_book"][c])
            assert f["class_subbook"][c] == [int(x) for x in d[f"floor/{i}/class_subbook"][c][:1 << f["class_subs"][c]]]
        want = [int(x) for x in d[f"floor/{i}/postlist"][:len(f["postlist"])]]
        want[1] = 1 << ilog(want[1] - 1)     # the range is sent as a bit count (lib/floor1.c:105, :164): 12 reads back as 16
        assert f["postlist"] == want
    for i, r in enumerate(u["residues"]):
        head = [int(x) for x in d[f"residue/{i}/head"]]
        assert [r["type"], r["begin"], r["end"], r["grouping"], r["partitions"], r["groupbook"]] == \
            [head[0], head[1], head[2], head[3], head[4], head[6]]
        assert r["secondstages"] == [int(x) for x in d[f"residue/{i}/secondstages"][:r["partitions"]]]
        assert r["booklist"] == [int(x) for x in d[f"residue/{i}/booklist"][:len(r["booklist"])]]
    for i, m in enumerate(u["maps"]):
        assert m["submaps"] == int(d[f"map/{i}/submaps"][0])
        steps = int(d[f"map/{i}/coupling_steps"][0])
        assert m["coupling"] == [(int(d[f"map/{i}/coupling_mag"][k]), int(d[f"map/{i}/coupling_ang"][k])) for k in range(steps)]
        assert m["chmuxlist"] == [int(x) for x in d[f"map/{i}/chmuxlist"][:ch]]
        assert m["floorsubmap"] == [int(x) for x in d[f"map/{i}/floorsubmap"][:m["submaps"]]]
        assert m["residuesubmap"] == [int(x) for x in d[f"map/{i}/residuesubmap"][:m["submaps"]]]
    for i, md in enumerate(u["modes"]):
        assert list(md) == [int(x) for x in d[f"mode/{i}"]]
    setup.close()


def test_ogg_pages_round_trip():
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(5)
    sizes = [30, 74, 4225, 0, 1, 254, 255, 256, 509, 510, 511, 3000, 70000, 12] + [int(x) for x in rng.integers(1, 900, 400)]
    packets = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in sizes]
    os_ = v.OggStream(0x1234abcd)
    blob = b""
    gp = 0
    for i, p in enumerate(packets):
        gp += 1024 if i >= 3 else 0
        os_.packetin(p, gp if i >= 3 else 0, eos=(i == len(packets) - 1))
        if i == 2:
            blob += b"".join(os_.pages(flush=True))      # headers flushed: audio starts on a fresh page
        else:
            blob += b"".join(os_.pages())
    blob += b"".join(os_.pages(flush=True))
    pages = parse_pages(blob)
    assert packets_of(pages) == packets
    assert [pg["seq"] for pg in pages] == list(range(len(pages)))
    assert all(pg["serial"] == 0x1234abcd for pg in pages)
    assert pages[0]["flags"] & 2 and not any(pg["flags"] & 2 for pg in pages[1:])        # b_o_s on the first page only
    assert pages[-1]["flags"] & 4 and not any(pg["flags"] & 4 for pg in pages[:-1])      # e_o_s on the last page only
    assert pages[0]["lacing"] == [30]                                                    # first page = first packet alone
    assert all(len(pg["lacing"]) <= 255 for pg in pages)
    # granule position of a page = that of the last packet ENDING on it, -1 if none ends there
    gps, g = [], 0
    for i in range(len(packets)):
        g += 1024 if i >= 3 else 0
        gps.append(g if i >= 3 else 0)
    done = 0
    for pg in pages:
        ends = sum(1 for lv in pg["lacing"] if lv < 255)
        done += ends
        assert pg["granule"] == (gps[done - 1] if ends else -1)
    os_.close()


def test_page_checksums_agree():
    """the tests' two checksums (table and bitwise, tests/ogg_pages.py) and the product's, which the corpora no longer
    borrow: on no bytes, on one byte, and on every page of a file with its checksum field zeroed"""
    from vorbis_aotuv_lancer_amd.stream import _page_crc
    from tests.ogg_demux_batch import six_packet_file
    pages = split_pages(six_packet_file()[0])
    assert len(pages) >= 3
    for p in pages:
        p[22:26] = b"\0\0\0\0"
    for data in [b"", b"\x5a"] + [bytes(p) for p in pages]:
        assert page_crc(data) == crc_bitwise(data) == _page_crc(data), len(data)
    assert page_crc(b"\x5a") != 0


def test_header_bytes_equal_the_oracles(oracle):
    """The three header packets of every shipped setup, packed by the product from the mode pack
    (csrc/capi_stream.cpp) and by the oracle from its own setup structs (oracle/orc_headers.c, restating
    lib/info.c:500-617, lib/codebook.c:158-275, floor1_pack, res0_pack, mapping0_pack): byte for byte."""
    import ctypes as C
    import glob
    import re
    import vorbis_aotuv_lancer_amd as v
    from tests import orc
    lib = oracle.lib
    lib.orc_header_packets.restype = C.c_long
    lib.orc_header_packets.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_void_p, C.c_long,
                                       C.POINTER(C.c_long)]
    comments = ["ENCODER=test", "TITLE=header parity", ""]
    arr = (C.c_char_p * len(comments))(*[c.encode() for c in comments])
    packs = sorted(glob.glob(os.path.join(os.path.dirname(v.LIB_PATH), "data", "mode_*.vpk")))
    assert len(packs) >= 20
    for path in packs:
        m = re.match(r"mode_(\d+)ch_(\d+)_(q|b)(-?[\d.]+?)(?:_max(\d+))?(?:_min(\d+))?\.vpk", os.path.basename(path))
        ch, rate = int(m.group(1)), int(m.group(2))
        if m.group(3) == "q":
            kw = dict(q=float(m.group(4)))
            setup = v.Setup(ch, rate, float(m.group(4)))
        else:
            br = (int(m.group(5) or -1), int(m.group(4)), int(m.group(6) or -1))
            kw = dict(bitrate=br)
            setup = v.Setup(ch, rate, bitrate=br)
        mine = v.header_packets(setup, comments)
        osetup = orc.Setup(oracle, ch, rate, **kw)
        lens = (C.c_long * 3)()
        total = lib.orc_header_packets(osetup.h, None, arr, len(comments), None, 0, lens)
        assert total > 0
        buf = (C.c_ubyte * total)()
        assert lib.orc_header_packets(osetup.h, None, arr, len(comments), buf, total, lens) == total
        raw = bytes(buf)
        theirs = [raw[:lens[0]], raw[lens[0]:lens[0] + lens[1]], raw[lens[0] + lens[1]:]]
        for k in range(3):
            assert mine[k] == theirs[k], (os.path.basename(path), k, len(mine[k]), len(theirs[k]))
        setup.close()
