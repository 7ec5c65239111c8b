"""The decoder's host side against an independent, spec-level model (tests/vorbis_model.py), on streams this project's
encoder never writes (no GPU).

First the model itself: on the PARITY classes it must reproduce the oracle's encode-side captures exactly, on the
reference's packet dumps it must equal the host unpack, and its dequantiser must reproduce the reference's self-test
vectors.  Then header round trips, the generated corpus (host unpack = model, bit for bit, on every packet), a
coverage assertion that names what a later change of the generator dropped, and setups the decoder must reject."""
import copy
import os

import numpy as np
import pytest

from tests import orc
from tests import vorbis_model as vm
from tests.decode_packets import (DATA, DUMPS, EBADHEADER, EIMPL, NAMES, PACKS, PARITY, QUANTLIST, Q_DELTA, Q_MIN,
                                  TEST4, TEST5, dump_packets, family, floor_expected, fromdB, headers_of,
                                  oracle_packets, pack_setup, residue_coded, unpack_differs, unpack_headers, vpk)


# ---- the model is checked first ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,rate,q", PARITY)
def test_model_matches_the_oracle_captures_exactly(oracle, ch, rate, q):
    """the comparisons of test_unpack_matches_the_oracle_captures_exactly, made for the model"""
    h = headers_of(ch, rate, q)
    ref = unpack_headers(*h)
    model = vm.Model(ref, fromdB())
    blocks = oracle_packets(oracle, ch, rate, q)
    pack = vpk.read_vpk(os.path.join(DATA, orc.mode_pack_name(ch, rate, q)))
    enc_x1 = [int(pack[f"floor/{i}/postlist"][1]) for i in range(len(ref["floors"]))]
    kinds = set()
    for k, b in enumerate(blocks):
        r = model.decode(b["packet"])
        assert r["status"] == 0, f"packet {k}"
        mode, W, lW, nW = r["info"]
        n = ref["blocksizes"][W] // 2
        assert W == b["W"] and (not W or (lW, nW) == (b["lW"], b["nW"])), f"packet {k}"
        kinds.add((b["lW"], b["W"], b["nW"]) if W else (0, 0, 0))
        assert list(r["used"]) == list(b["nonzero"]), f"packet {k}: floor-used flags"
        assert list(r["used_before"]) == [int(x) for x in b["post_valid"]], f"packet {k}: floor-coded flags"
        np.testing.assert_array_equal(r["floor_index"][:, :n], floor_expected(ref, enc_x1, mode, b["ilogmask"], n),
                                      err_msg=f"packet {k}: floor index")
        want = np.where(residue_coded(ref, mode, ch, n, b["nonzero"]), b["residue"].astype(np.float32), np.float32(0))
        np.testing.assert_array_equal(r["residue"][:, :n], want, err_msg=f"packet {k}: residue")
        assert not r["floor_index"][:, n:].any() and not r["residue"][:, n:].any()
    if ref["blocksizes"][0] != ref["blocksizes"][1]:
        assert {(0, 0, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)} <= kinds, kinds


@pytest.mark.parametrize("ch,rate,q,golden", DUMPS)
def test_model_equals_host_unpack_on_the_reference_dumps(ch, rate, q, golden):
    import vorbis_aotuv_lancer_amd as v
    h = headers_of(ch, rate, q)
    ds = v.DecodeSetup(h)
    model = vm.Model(unpack_headers(*h), fromdB())
    packets = dump_packets(golden)
    assert len(packets) > 400
    for k in range(len(packets)):
        diff = unpack_differs(ds.unpack(packets[k]), model.decode(packets[k]))
        assert diff is None, f"packet {k}: {diff}"
    ds.close()


def test_model_dequantiser_on_the_references_selftest_vectors():
    # 27 entries as a complete tree: 5 words of 4 bits and 22 of 5
    book = {"dim": 3, "entries": 27, "lengthlist": [4] * 5 + [5] * 22, "maptype": 1, "q_min": Q_MIN & 0xffffffff,
            "q_delta": Q_DELTA & 0xffffffff, "q_quant": 4, "q_sequencep": 0, "quantlist": QUANTLIST}
    assert (vm.float32_unpack(book["q_min"]), vm.float32_unpack(book["q_delta"])) == (-3.0, 1.0)
    assert vm.lookup1_values(27, 3) == 3 and vm.lookup1_values(3, 4) == 1
    assert vm.Book(book).vals.ravel().tolist() == TEST4
    assert vm.Book(dict(book, q_sequencep=1)).vals.ravel().tolist() == TEST5
    for entries, dim in [(6561, 8), (625, 4), (81, 2), (289, 2), (3125, 5), (7, 3), (8, 3), (9, 3), (1, 5)]:
        q = vm.lookup1_values(entries, dim)
        assert q ** dim <= entries < (q + 1) ** dim


def test_codeword_assignment_on_the_specifications_example():
    """spec 3.2.1: lengths 2 4 4 4 4 2 3 3 -> 00 0100 0101 0110 0111 10 110 111"""
    b = vm.Book({"dim": 1, "entries": 8, "lengthlist": [2, 4, 4, 4, 4, 2, 3, 3], "maptype": 0})
    got = ["".join(map(str, b.code[i])) for i in range(8)]
    assert got == ["00", "0100", "0101", "0110", "0111", "10", "110", "111"]


# ---- header round trips ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pack", PACKS)
def test_pack_headers_rewrites_every_shipped_setup_header_byte_for_byte(pack):
    import vorbis_aotuv_lancer_amd as v
    setup, _ = pack_setup(v, pack)
    h = v.header_packets(setup, ["TITLE=round trip"])
    assert vm.pack_headers(unpack_headers(*h)) == tuple(h)
    setup.close()


@pytest.mark.parametrize("k", range(len(vm.CORPUS)), ids=NAMES)
def test_generated_headers_round_trip(k):
    setup, coding = vm.build_corpus_setup(k)
    assert unpack_headers(*vm.pack_headers(setup, coding)) == setup


@pytest.mark.parametrize("k", range(len(vm.CORPUS)), ids=NAMES)
def test_host_unpack_equals_the_model_on_the_generated_corpus(k):
    setup, _, _, _, rows, facts, bad = family(k)
    assert facts == ((len(setup["books"]), len(setup["floors"]), len(setup["residues"]), len(setup["maps"])),
                     setup["blocksizes"], len(setup["modes"]), setup["channels"])
    labels = {l.split("[")[0].split("+")[0].rstrip("0123456789") for l, _, _ in rows}
    assert {"writer", "random", "empty", "header"} <= labels
    assert any("[:" in l for l, _, _ in rows) and any("+garbage" in l for l, _, _ in rows)
    assert not bad, f"{len(bad)} of {len(rows)} packets differ: " + "; ".join(bad[:5])


# ---- coverage --------------------------------------------------------------------------------------------------------
def features(setup, coding):
    """the rows of the coverage table a setup supplies"""
    F = set()
    bs, ch = setup["blocksizes"], setup["channels"]
    books = setup["books"]
    F.add(f"block sizes {bs[0]}/{bs[1]}")
    F.add(f"{ch} channels")
    F.add(f"{vm.ilog(len(setup['modes']) - 1)} mode bits")
    if len(setup["modes"]) == 64:
        F.add("64 modes")
    maps_used = [md[3] for md in setup["modes"]]
    if len(maps_used) != len(set(maps_used)):
        F.add("modes sharing a mapping")
    for i, b in enumerate(books):
        L = b["lengthlist"]
        used = [l for l in L if l]
        F.add(f"book header coding {coding[i]}")
        if len(used) == 1:
            F.add("single-entry book")
        if any(24 <= l < 32 for l in L):
            F.add("codeword length 24-31")
        if 32 in L:
            F.add("codeword length 32")
        nz = [j for j, l in enumerate(L) if l]
        if len(used) > 1 and any(L[j] == 0 for j in range(nz[0], nz[-1])):
            F.add("sparse book with unused entries between used ones")
    for mi, m in enumerate(setup["maps"]):
        flags = {md[0] for md in setup["modes"] if md[3] == mi}
        if not flags:
            continue
        if ch == 1 and not m["coupling"]:
            F.add("mono, coupling-free")
        if m["submaps"] >= 3:
            F.add("3 or more submaps")
        if m["submaps"] == 16:
            F.add("16 submaps")
        steps = len(m["coupling"])
        if steps not in (0, 1, 4):
            F.add("coupling steps other than 0, 1, 4")
        for c in range(ch):
            if sum((c in p) for p in m["coupling"]) >= 3:
                F.add("a channel in three or more coupling steps")
        for sm in range(m["submaps"]):
            chans = [c for c in range(ch) if m["chmuxlist"][c] == sm]
            if not chans:
                continue
            f, r = setup["floors"][m["floorsubmap"][sm]], setup["residues"][m["residuesubmap"][sm]]
            F.add(f"floor multiplier {f['mult']}")
            if len(flags) == 2 and bs[0] != bs[1] and f["postlist"][1] > bs[0] // 2:
                F.add("floor shared by both block sizes with postlist[1] above n")
            if any(all(x < 0 for x in sb) for sb in f["class_subbook"]):
                F.add("floor class with no books")
            F.add(f"residue type {r['type']}")
            if r["begin"] > 0:
                F.add("residue begin > 0")
            if r["end"] <= r["begin"]:
                F.add("residue end <= begin")
            for flag in flags:
                size = bs[flag] // 2 * (len(chans) if r["type"] == 2 else 1)
                F.add("residue end " + ("below" if r["end"] < size else "at" if r["end"] == size else "above")
                      + " the block")
                nparts = max(min(r["end"], size) - r["begin"], 0) // r["grouping"]
                gd = books[r["groupbook"]]["dim"]
                F.add(f"group book dimension {gd}")
                if gd > 1 and nparts % gd:
                    F.add(f"group book dimension {gd} with a partition count that is not a multiple of it")
            if r["grouping"] == 1:
                F.add("residue grouping 1")
            if 0 in r["secondstages"]:
                F.add("residue class with no books")
            for c in r["secondstages"]:
                if c >= 16:
                    F.add("cascade stages 5-8")
                if c and any(not (c >> s_) & 1 for s_ in range(vm.ilog(c))):
                    F.add("cascade mask with a gap")
            for bi in r["booklist"]:
                b = books[bi]
                F.add(f"stage book maptype {b['maptype']}")
                if b["q_sequencep"]:
                    F.add("stage book with q_sequencep = 1")
                if r["grouping"] % b["dim"]:
                    F.add(f"residue {r['type']}: book dimension that does not divide the grouping")
                if r["type"] == 2 and (b["dim"] % len(chans) and len(chans) % b["dim"]):
                    F.add("residue 2: book dimension against the channel count, neither divides the other")
    return F


REQUIRED = (
    [f"block sizes {a}/{b}" for a, b in vm.PAIRS] + [f"{c} channels" for c in range(1, 9)] +
    [f"{b} mode bits" for b in range(7)] + ["64 modes", "modes sharing a mapping", "mono, coupling-free"] +
    [f"book header coding {c}" for c in ("ordered", "dense", "sparse")] +
    ["single-entry book", "codeword length 24-31", "codeword length 32",
     "sparse book with unused entries between used ones", "3 or more submaps", "16 submaps",
     "coupling steps other than 0, 1, 4", "a channel in three or more coupling steps"] +
    [f"floor multiplier {m}" for m in (1, 2, 3, 4)] +
    ["floor shared by both block sizes with postlist[1] above n", "floor class with no books"] +
    [f"residue type {t}" for t in (0, 1, 2)] +
    ["residue begin > 0", "residue end <= begin", "residue end below the block", "residue end at the block",
     "residue end above the block", "residue grouping 1", "residue class with no books", "cascade stages 5-8",
     "cascade mask with a gap", "stage book maptype 1", "stage book maptype 2", "stage book with q_sequencep = 1"] +
    [f"group book dimension {d}" for d in (1, 2, 3, 4)] +
    [f"group book dimension {d} with a partition count that is not a multiple of it" for d in (2, 3, 4)] +
    [f"residue {t}: book dimension that does not divide the grouping" for t in (0, 1, 2)] +
    ["residue 2: book dimension against the channel count, neither divides the other"])


# what each family is in the corpus for: checked on the family's own setup, so that a family that is removed, or
# that a change of the generator hollows out, is named
PURPOSE = {
    "pair_256_256_grouping1": ["block sizes 256/256", "residue grouping 1", "3 channels"],
    "pair_256_512_res0": ["block sizes 256/512", "residue type 0",
                          "residue 0: book dimension that does not divide the grouping"],
    "pair_256_1024_res2_odd_dims": ["block sizes 256/1024", "residue type 2",
                                    "residue 2: book dimension that does not divide the grouping",
                                    "residue 2: book dimension against the channel count, neither divides the other"],
    "pair_256_2048_maptype2": ["block sizes 256/2048", "stage book maptype 2"],
    "pair_256_4096_shared_floor": ["block sizes 256/4096", "mono, coupling-free", "modes sharing a mapping",
                                   "floor shared by both block sizes with postlist[1] above n",
                                   "residue end above the block"],
    "pair_512_512_mult1_mult3": ["block sizes 512/512", "floor multiplier 1", "floor multiplier 3", "4 channels",
                                 "a channel in three or more coupling steps"],
    "pair_512_1024_submaps": ["block sizes 512/1024", "3 or more submaps", "floor multiplier 4", "8 channels",
                              "2 mode bits"],
    "pair_512_2048_begin_end": ["block sizes 512/2048", "residue begin > 0", "residue end below the block",
                                "4 mode bits"],
    "pair_512_4096_long_codewords": ["block sizes 512/4096", "codeword length 24-31", "codeword length 32",
                                     "book header coding ordered"],
    "pair_1024_1024_seq": ["block sizes 1024/1024", "stage book with q_sequencep = 1", "5 channels", "5 mode bits"],
    "pair_1024_2048_stages_5_8": ["block sizes 1024/2048", "cascade stages 5-8", "cascade mask with a gap"],
    "pair_1024_4096_group_dims": ["block sizes 1024/4096", "group book dimension 1", "group book dimension 3",
                                  "group book dimension 3 with a partition count that is not a multiple of it",
                                  "6 channels"],
    "pair_2048_2048_end_le_begin": ["block sizes 2048/2048", "residue end <= begin", "counter empty_residue_range"],
    "pair_2048_4096_end_above": ["block sizes 2048/4096", "residue end above the block", "7 channels"],
    "pair_4096_4096_single_books": ["block sizes 4096/4096", "single-entry book", "counter single_entry_book_read"],
    "modes_64": ["64 modes", "6 mode bits"],
    "modes_1": ["0 mode bits"],
    "modes_5_submaps_16": ["16 submaps", "3 mode bits", "a packet with a mode index past the last mode"],
    "group_dim4_ragged": ["group book dimension 4 with a partition count that is not a multiple of it"],
    "sparse_32bit": ["sparse book with unused entries between used ones", "codeword length 32",
                     "book header coding sparse"],
}


def test_every_family_supplies_what_it_is_there_for():
    missing = [f"family {name} is not in the corpus" for name in PURPOSE if name not in NAMES]
    assert sorted(NAMES) == sorted(set(NAMES)) and not [n for n in NAMES if n not in PURPOSE], "a family without a purpose"
    for k, name in enumerate(NAMES):
        setup, coding, _, counters, rows, _, _ = family(k)
        have = features(setup, coding) | {f"counter {c}" for c in vm.COUNTERS if counters[c]}
        if any(l == "mode_past_last" for l, _, _ in rows):
            have.add("a packet with a mode index past the last mode")
        missing += [f"{name}: {f}" for f in PURPOSE[name] if f not in have]
    assert not missing, "; ".join(missing)


def test_the_corpus_covers_every_counter_and_every_table_row():
    have, total = set(), {c: 0 for c in vm.COUNTERS}
    labels = set()
    for k, name in enumerate(NAMES):
        setup, coding, _, counters, rows, _, _ = family(k)
        have |= features(setup, coding)
        for c in vm.COUNTERS:
            total[c] += counters[c]
        labels |= {l for l, _, _ in rows}
    missing = [f for f in REQUIRED if f not in have] + [f"counter {c}" for c in vm.COUNTERS if not total[c]]
    if "mode_past_last" not in labels:
        missing.append("a packet with a mode index past the last mode")
    assert not missing, "the generated corpus no longer covers: " + "; ".join(missing)


# ---- setups the decoder must reject ------------------------------------------------------------------------------------
def status_of(setup, coding=None, **kw):
    import vorbis_aotuv_lancer_amd as v
    return v.DecodeSetup.status(vm.pack_headers(setup, coding, **kw))


def fresh(k):
    setup, coding = vm.build_corpus_setup(k)
    assert status_of(setup, coding) == 0
    return copy.deepcopy(setup), list(coding)


def test_broken_setups_are_ebadheader():
    # duplicate post
    s, c = fresh(1)
    f = next(f for f in s["floors"] if len(f["postlist"]) >= 4)
    f["postlist"][3] = f["postlist"][2]
    assert status_of(s, c) == EBADHEADER
    s, c = fresh(1)
    s["floors"][0]["postlist"][-1] = 0                         # ... of the implicit first post
    assert status_of(s, c) == EBADHEADER
    # magnitude = angle
    s, c = fresh(1)
    s["maps"][0]["coupling"] = [(1, 1)]
    assert status_of(s, c) == EBADHEADER
    # mux >= submaps
    s, c = fresh(NAMES.index("pair_512_1024_submaps"))
    assert s["maps"][0]["submaps"] == 5
    s["maps"][0]["chmuxlist"][0] = 5
    assert status_of(s, c) == EBADHEADER
    # book indices out of range: stage book, group book, floor class book and sub-book
    s, c = fresh(1)
    s["residues"][0]["booklist"][0] = len(s["books"])
    assert status_of(s, c) == EBADHEADER
    s, c = fresh(1)
    s["residues"][0]["groupbook"] = len(s["books"])
    assert status_of(s, c) == EBADHEADER
    s, c = fresh(1)
    f = next(f for f in s["floors"] if any(x >= 0 for sb in f["class_subbook"] for x in sb))
    sb = next(sb for sb in f["class_subbook"] if any(x >= 0 for x in sb))
    sb[[x >= 0 for x in sb].index(True)] = len(s["books"])
    assert status_of(s, c) == EBADHEADER
    # group book too small: 2 entries of dimension 2 for >= 2 classifications
    s, c = fresh(1)
    s["books"].append({"dim": 2, "entries": 2, "lengthlist": [1, 1], "maptype": 0})
    c.append("dense")
    assert status_of(s, c) == 0
    assert s["residues"][0]["partitions"] >= 2
    s["residues"][0]["groupbook"] = len(s["books"]) - 1
    assert status_of(s, c) == EBADHEADER
    # stage book without a value mapping
    s, c = fresh(1)
    gb = s["residues"][0]["groupbook"]
    assert s["books"][gb]["maptype"] == 0
    s["residues"][0]["booklist"][0] = gb
    assert status_of(s, c) == EBADHEADER
    # over- and under-populated trees with more than one entry (a book nothing refers to)
    for lengths in ([1, 1, 1], [1, 2, 2, 2], [2, 2, 2], [1, 3, 3], [32, 32]):
        s, c = fresh(1)
        s["books"].append({"dim": 1, "entries": len(lengths), "lengthlist": lengths, "maptype": 0})
        c.append("dense")
        assert status_of(s, c) == EBADHEADER, lengths
    # stage book of dimension 0 (the documented deviation: the reference would divide by it)
    s, c = fresh(1)
    s["books"].append({"dim": 0, "entries": 2, "lengthlist": [1, 1], "maptype": 2, "q_min": 0, "q_delta": 0,
                       "q_quant": 1, "q_sequencep": 0, "quantlist": []})
    c.append("dense")
    assert status_of(s, c) == 0
    s["residues"][0]["booklist"][0] = len(s["books"]) - 1
    assert status_of(s, c) == EBADHEADER
    # framing bit of the setup header
    s, c = fresh(1)
    assert status_of(s, c, framing=0) == EBADHEADER


def test_unsupported_setups_are_eimpl():
    s, c = fresh(1)
    assert status_of(s, c, floor_types=[0] * len(s["floors"])) == EIMPL
    s, c = fresh(NAMES.index("modes_1"))                                            # one submap, no coupling
    assert not s["maps"][0]["coupling"] and s["maps"][0]["submaps"] == 1
    s["channels"] = 9
    s["maps"][0]["chmuxlist"] = [0] * 9
    assert status_of(s, c) == EIMPL
    for bs in ([128, 2048], [256, 8192], [128, 128], [8192, 8192]):
        s, c = fresh(1)
        s["blocksizes"] = bs
        assert status_of(s, c) == EIMPL, bs


def test_window_table_is_the_vorbis_window():
    """The PCM tests of test_decoder_synthetic_gpu.py overlap-add with the float64 formula; the table the kernels read
    must be that formula.  It holds the reference's decimal constants rounded to float32, so it may miss the formula
    by up to one float32 step at 1.0 (2^-24); measured: 2.98e-8 = 2^-25 at every size."""
    import vorbis_aotuv_lancer_amd as v
    for bs in (256, 512, 1024, 2048, 4096):
        w = v.window_table(bs)
        assert w.dtype == np.float32 and w.shape == (bs // 2,)
        err = np.abs(w.astype(np.float64) - vm.vorbis_window64(bs // 2)).max()
        print(f"window {bs}: max |table - formula| = {err:.3g}")
        assert err <= 2.0 ** -24
