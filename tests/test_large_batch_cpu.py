"""The large-batch matrix (tests/large_batch.py) does what it is for: from the oracle and the product's size query
alone, no GPU.  Per case: the schedule holds every block type of the class, every call takes every large form the block
type has, and the signals still take the branches they are in the case for (the witnesses of tests/test_reach_cpu.py and
tests/test_images_cpu.py, on the streams as the case cuts them)."""
import numpy as np
import pytest

from tests import large_batch as lb
from tests.large_batch import CASE_IDS, CASES


def bits():
    from vorbis_aotuv_lancer_amd import encoder as e
    return e


def test_matrix_shape():
    assert len(CASES) == 13 and len(set(CASE_IDS)) == 13
    assert all(1 <= len(c["signals"]) <= 4 and c["seconds"] <= 2.0 for c in CASES)


def test_query_is_monotone_and_few_selects_the_small_forms():
    """a device-built round's batch (few = 1) takes no large form at any size, and bit 4 only where slices of 64 bins fit"""
    import vorbis_aotuv_lancer_amd as v
    e = bits()
    for ch in (1, 2, 6, 8):
        for n in (128, 256, 512, 1024, 2048):
            for mode in range(4):
                last = 0
                for nsb in [1, 2, 63, 64, 65] + [1 << s for s in range(7, 21)] + [(1 << s) + 1 for s in range(7, 21)]:
                    assert v.batch_variants(mode, n, ch, nsb, few=True) & e.LARGE_BATCH_BITS == 0, (ch, n, mode, nsb)
                for nsb in sorted([1 << s for s in range(0, 21)] + [(1 << s) + 1 for s in range(0, 21)]):
                    m = v.batch_variants(mode, n, ch, nsb) & e.LARGE_BATCH_BITS
                    assert m & last == last, (ch, n, mode, nsb)          # a form once large stays large
                    last = m
                assert last == lb.wanted_bits(mode)
                assert v.batch_variants(mode, n, ch, 1) & e.LARGE_BATCH_BITS == 0
                assert bool(v.batch_variants(mode, n, ch, 1) & e.MIX_MAKES_FIT_WORDS) == (mode != 0)


def test_pick_R_is_minimal_and_leaves_partial_tiles():
    for c in CASES:
        R, ch, sizes = lb.R_of(c), c["ch"], lb.blocksizes(c)
        assert R % 64 and (R * ch) % 64
        for N in sizes:
            for mode in lb.block_types(c):
                for j in range(1, len(c["signals"]) + 1):
                    assert lb.call_mask(mode, N // 2, ch, R * j, c["sub_batches"]) & lb.wanted_bits(mode) == lb.wanted_bits(mode)
        # ... and no smaller replica count does: some call of R0 < R copies of one signal misses a large form
        R0 = R - 1
        while R0 % 64 == 0 or (R0 * ch) % 64 == 0:
            R0 -= 1
        assert any(lb.call_mask(m, N // 2, ch, R0 * j, c["sub_batches"]) & lb.wanted_bits(m) != lb.wanted_bits(m)
                   for N in sizes for m in range(4) for j in range(1, len(c["signals"]) + 1)), (c["name"], R, R0)
    # the sliced case needs more than twice the streams: whole tiles are dealt, so the smaller slice is what counts
    assert lb.R_of(CASES[-1]) >= 2 * lb.R_of(CASES[0]) - 64
    assert min(lb.slices_of(lb.R_of(CASES[-1]), 2)) * 2 <= lb.R_of(CASES[-1])


def test_replicated_schedule_layout():
    streams = [[dict(block_mode=m, N=2048) for m in (3, 3, 2, 0)], [dict(block_mode=m, N=2048) for m in (3, 2, 0)],
               [dict(block_mode=m, N=2048) for m in (3, 3, 3, 3, 1)]]
    sched = lb.replicated_schedule(streams, 5)
    assert [(k, m, p) for k, m, p, _ in sched] == [(0, 3, [0, 1, 2]), (1, 2, [1]), (1, 3, [0, 2]), (2, 0, [1]), (2, 2, [0]), (2, 3, [2]),
                                                   (3, 0, [0]), (3, 3, [2]), (4, 1, [2])]
    for k, m, present, ids in sched:
        assert len(ids) == 5 * len(present) and np.all(np.diff(ids) > 0) and ids.dtype == np.int32
        assert [int(s) % 3 for s in ids] == present * 5 and ids.max() < 15
        assert ids[:len(present)].tolist() == present                     # the first copies lead


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_schedule_reaches_every_block_type_in_its_large_forms(oracle, c):
    e = bits()
    streams = lb.streams_of(oracle, c)
    seen = lb.schedule_masks(c, streams, lb.R_of(c))
    assert set(seen) == set(lb.block_types(c)), (c["name"], sorted(seen))
    for mode, masks in seen.items():
        for m in masks:
            assert m & e.LARGE_BATCH_BITS == lb.wanted_bits(mode), (c["name"], mode, m)
    if c["q"] is not None and c["q"] < 0:
        # blocks of 4096: slices of 128 bins do not fit the tile, the floor fit's words come from their own pass, which
        # the small batches run for impulse blocks only
        assert lb.blocksizes(c)[1] == 4096
        for mode in (2, 3):
            assert all(not m & e.MIX_MAKES_FIT_WORDS for m in seen[mode]), seen[mode]
        assert all(m & e.MIX_MAKES_FIT_WORDS for m in seen[1])
    else:
        assert all(bool(m & e.MIX_MAKES_FIT_WORDS) == (mode != 0) for mode, masks in seen.items() for m in masks)
    print(f"{c['name']}: R = {lb.R_of(c)}, " + ", ".join(f"type {m}: masks {sorted(s)}" for m, s in sorted(seen.items())))


# ---- witnesses ------------------------------------------------------------------------------------------------------------
def named(oracle, c, name):
    return lb.streams_of(oracle, c)[[n for n, _ in c["signals"]].index(name)]


def poste_blocks(blks):
    return sum(bool((b["poste"] > 0).any()) for b in blks)


def tied_rows(blks, mag=0, ang=1):
    """blocks whose angle row is all zero under a magnitude row that is not: the pair was tied in every bin"""
    return sum(bool(b["residue"][mag].any() and not b["residue"][ang].any()) for b in blks)


def minus_twice(blks, mag=0, ang=1):
    return sum(int(((b["residue"][ang] != 0) & (b["residue"][ang] == -2 * np.abs(b["residue"][mag]))).sum()) for b in blks)


def case_named(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if any(n == "decaying_hits" for n, _ in c["signals"])])
def test_decaying_hits_set_the_post_echo_detector_off(oracle, name):
    c = case_named(name)
    n = poste_blocks(named(oracle, c, "decaying_hits"))
    if max(lb.blocksizes(c)) < 2048:
        assert n == 0           # the detector turns every block below 2048 down (tests/test_reach_cpu.py)
    else:
        assert n >= 3, (name, n)


def test_witnesses_stereo_q5(oracle):
    c = case_named("2ch_44100_q0.5_reach")
    assert minus_twice(named(oracle, c, "inverted")) >= 1000 and tied_rows(named(oracle, c, "inverted")) == 0
    faint = named(oracle, c, "faint_noise")
    for modes in ((3,), (0, 1)):
        assert any(b["block_mode"] in modes and not b["post_valid"].any() for b in faint)
    assert any(b["post_valid"].all() for b in faint)
    clicks = named(oracle, c, "click_trains")
    assert sum(b["block_mode"] == 0 for b in clicks) >= 20 and any(b["N"] == 256 for b in clicks)
    c = case_named("2ch_44100_q0.5_edges")
    assert tied_rows(named(oracle, c, "dual_mono")) >= 50
    gated = named(oracle, c, "gated_bands")
    assert any(b["post_valid"].tolist() == [0, 1] and b["nonzero"].tolist() == [1, 1] for b in gated)
    tail = named(oracle, c, "zero_tail")
    assert not tail[0]["post_valid"].any() and not tail[-1]["post_valid"].any() and any(b["post_valid"].all() for b in tail)


def test_witnesses_lowest_quality(oracle):
    c = case_named("2ch_44100_q-0.1")
    loud = named(oracle, c, "overdriven_noise")
    # fitline_y0_above_1023: a fitted post at the top of the floor's range, in long and in short blocks
    top = [b for b in loud for x in range(2) if b["post_valid"][x] and ((b["post"][x] & 0x7fff) == 1023).any()]
    assert top and {b["N"] for b in top} == {512, 4096}
    assert any(b["N"] == 512 and b["block_mode"] == 0 for b in named(oracle, c, "click_trains"))
    left = named(oracle, c, "hard_left")
    assert all(b["post_valid"][1] == 0 for b in left) and any(b["post_valid"][0] for b in left)


def test_witnesses_coupled_51(oracle):
    c = case_named("6ch_48000_q0.3")
    steps = lb.pack_of(c)
    pairs = [(int(steps["map/0/coupling_mag"][k]), int(steps["map/0/coupling_ang"][k])) for k in range(int(steps["map/0/coupling_steps"][0]))]
    assert (0, 1) in pairs
    assert minus_twice(named(oracle, c, "alt_sign"), 0, 1) >= 1000          # (0, 1): opposite channels, the last step to write row 1
    live = named(oracle, c, "one_live")
    assert all(not b["post_valid"][1:].any() for b in live) and any(b["post_valid"][0] for b in live)
    hits = [b for b in named(oracle, c, "decaying_hits") if (b["poste"] > 0).any()]
    assert any((b["poste"] > 0).any() and (b["poste"] < 0).any() for b in hits)
    c = case_named("6ch_48000_q0.1")
    assert any(0 < b["post_valid"][:5].sum() < 5 for b in named(oracle, c, "gated_bands"))
    front = named(oracle, c, "front_same_rest_independent")
    mag, ang = pairs[0]
    assert all(np.array_equal(b["mdct_raw"][mag].view(np.uint32), b["mdct_raw"][ang].view(np.uint32)) for b in front)
    assert tied_rows(front, mag, ang) >= 1


def test_witnesses_other_classes(oracle):
    c = case_named("2ch_22050_q0.5")
    swap = named(oracle, c, "swap_mid_stream")
    assert tied_rows(swap) >= 1 and minus_twice(swap) >= 1 and max(b["N"] for b in swap) == 1024
    c = case_named("1ch_8000_q0.5")
    assert {b["N"] for s in lb.streams_of(oracle, c) for b in s} == {512}
    c = case_named("8ch_44100_q0.5")
    same = named(oracle, c, "all_same")
    assert all(np.array_equal(b["mdct"][0].view(np.uint32), b["mdct"][x].view(np.uint32)) for b in same for x in range(1, 8))
    c = case_named("2ch_96000_q0.5")
    dither = named(oracle, c, "hard_left_dither")
    assert any(b["post_valid"].tolist() == [1, 0] for b in dither) or any(b["post_valid"].all() for b in dither)


def test_witnesses_managed(oracle):
    c = case_named("2ch_44100_b128000_max144000_min112000")
    cut = [b for b in named(oracle, c, "overdriven_noise") if len(b["packet"]) < b["blob_bytes"][b["choice"]]]
    assert len(cut) >= 3 and all(b["choice"] == 0 for b in cut)
    assert tied_rows(named(oracle, c, "swap_mid_stream")) >= 1
    c = case_named("2ch_44100_b256000")
    assert any(b["post_valid"].all() and b["blob_bytes"][0] == 1 and b["blob_bytes"][14] == 1 and b["blob_bytes"][7] > 4
               for b in named(oracle, c, "faint_noise"))


def test_encoded_posts_follow_the_packets_floor(oracle):
    """encoded_posts (the reference for `post`) against an independent reading: the first two posts of a block's packet
    are the quantised end posts, written with ilog(quant_q - 1) bits right after the header bits"""
    c = case_named("1ch_8000_q0.5")
    fl = lb.floors_of(c, 0)[0]
    posts, mult = fl[0], fl[1]
    qbits = {1: 8, 2: 7, 3: 7, 4: 6}[mult]
    checked = 0
    for b in named(oracle, c, "synth"):
        if not b["post_valid"][0]:
            continue
        p = lb.encoded_posts(b["post"][0], fl)
        assert p.shape == (posts,) and ((p & 0x7fff) < (1 << qbits)).all()
        word = int.from_bytes(b["packet"][:4], "little")
        # 1 bit packet type, 0 mode bits (one mode), no window flags (one block size), 1 bit "floor used"
        assert word & 1 == 0 and (word >> 1) & 1 == 1
        assert (word >> 2) & ((1 << qbits) - 1) == p[0] & 0x7fff and (word >> (2 + qbits)) & ((1 << qbits) - 1) == p[1] & 0x7fff
        checked += 1
    assert checked >= 10
