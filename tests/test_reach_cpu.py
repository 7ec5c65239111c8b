"""The reach corpus (tests/reach_signals.py) does what it is for — from the oracle's outputs alone, no GPU:

  * per signal, the block orders, detector values and flags its docstring promises (the witnesses below);
  * tools/oracle_reach.py on the corpus: every target that DESIGN.md §4 classifies as reached has a non-zero count;
  * the suite's own signals (the tool's `suite` corpus) never set the post-echo detector off, with one exception that
    is pinned here: the reference's windowed sine at 2ch 44100 q-0.1, one block, both channels above the clamp.  That
    is the gap the corpus closes.
"""
import multiprocessing
import os
import re
import sys

import numpy as np
import pytest

from tests import orc
from tests.encode_oracle import walk
from tests.reach_signals import REACH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle_reach  # noqa: E402

def entry(name):
    return next(e for e in REACH if e["name"] == name)


def blocks(oracle, name):
    e = entry(name)

    def pcm():
        x = e["make"](e["ch"], e["rate"])
        assert x.shape[1] <= 2 * e["rate"] and x.shape[1] % 1024 == 0
        return x
    return walk(oracle, e["ch"], e["rate"], e["q"], e["bitrate"], pcm, key=("reach", name))


def detector(pcm, mode, last_mode):
    """orc_postnoise_detection in float64 numpy -> (what it returns, the difference before the 0.1 rule or None, and
    whether it was the loud quarter that failed)"""
    nn = len(pcm)
    if mode != 2 or last_mode != 0 or nn < 2048:
        return np.float32(-1.0), None, False
    sn = nn >> 2
    a = np.abs(pcm.astype(np.float64))
    upt = np.cumsum(a[sn:2 * sn])[-1]                  # (cumsum adds in sample order, as the C loop does)
    unt = np.cumsum(a[2 * sn:3 * sn])[-1]
    if unt / sn > 0.01:
        return np.float32(-1.0), None, False
    upt *= upt
    unt *= unt
    unt *= 15
    if not upt > unt:
        return np.float32(-1.0), None, True
    raw = np.float32(upt - unt)
    return (raw if raw >= 0.1 else np.float32(-1.0)), raw, False


def detector_rows(blks):
    """per block: [(returned, raw, failed on the loud quarter)] per channel; asserts the oracle's capture is the same"""
    rows, last = [], 0          # (lW_block_mode starts at 0)
    for k, b in enumerate(blks):
        row = [detector(b["pcm"][c], b["block_mode"], last) for c in range(b["pcm"].shape[0])]
        got = np.array([r[0] for r in row], np.float32)
        assert np.array_equal(got.view(np.uint32), b["poste"].view(np.uint32)), (k, got, b["poste"])
        rows.append(row)
        last = b["block_mode"]
    return rows


@pytest.mark.parametrize("name", [e["name"] for e in REACH])
def test_detector_recomputed_from_pcm(oracle, name):
    detector_rows(blocks(oracle, name))


def test_decaying_hits_cover_the_detector_ranges(oracle):
    blks = blocks(oracle, "decaying_hits_2ch_44100_q0.5")
    rows = detector_rows(blks)
    flat = [r for row in rows for r in row]
    assert sum(r[0] > 0 for r in flat) >= 3
    assert any(r[0] >= 30 for r in flat)                               # VMIN(poste, 30) acts
    assert any(0.1 <= r[0] < 30 for r in flat)                         # ... and does not
    assert any(r[1] is not None and 0 < r[1] < 0.1 and r[0] == -1 for r in flat)        # (0, 0.1) is turned into -1
    # one block with poste > 0 in one channel while the other fails the detector on its loud quarter
    assert any(row[0][0] > 0 and row[1][0] == -1 and row[1][2] for row in rows)
    # what the arm leaves behind: npeak = -1 where the reduction was applied
    assert all((b["npeak"][c] == -1).any() for b in blks for c in range(2) if b["poste"][c] > 0)


@pytest.mark.parametrize("name,N", [("decaying_hits_1ch_44100_q0.1", 2048), ("decaying_hits_2ch_44100_q-0.1", 4096),
                                    ("decaying_hits_6ch_48000_q0.3", 2048), ("decaying_hits_2ch_44100_b128000", 2048)])
def test_decaying_hits_in_other_classes(oracle, name, N):
    blks = blocks(oracle, name)
    hit = [b for b in blks if (b["poste"] > 0).any()]
    assert len(hit) >= 3 and all(b["N"] == N for b in hit)
    if blks[0]["pcm"].shape[0] == 6:       # some channels of a block with, others without
        assert any((b["poste"] > 0).any() and (b["poste"] < 0).any() for b in hit)


def test_decaying_hits_below_2048_never_pass(oracle):
    blks = blocks(oracle, "decaying_hits_2ch_22050_q0.5")
    assert max(b["N"] for b in blks) == 1024
    asked = [k for k in range(1, len(blks)) if blks[k]["block_mode"] == 2 and blks[k - 1]["block_mode"] == 0]
    assert len(asked) >= 3                                             # the block order is there ...
    assert all((b["poste"] == -1).all() for b in blks)                 # ... and the size test turns every one down


def m3_history(blks):
    """(block_mode, lW_block_mode, lW_no, impadnum) as orc_offset_and_mix sees them, per block (orc_mapping.c, end of
    orc_mapping0_forward)"""
    out, last, no, impad = [], 0, 0, 0
    for b in blks:
        bm = b["block_mode"]
        out.append((bm, last, no, impad))
        if bm >= 2:
            impad = 0
        if last == 0 and bm == 1:
            impad = 1
        elif impad and impad < 8:
            impad += 1
        no = no + 1 if last == bm else 1
        last = bm
    return out


@pytest.mark.parametrize("name,N", [("click_trains_2ch_44100_q-0.1", 512), ("click_trains_2ch_44100_q0.5", 256)])
def test_click_trains_short_block_history(oracle, name, N):
    blks = blocks(oracle, name)
    hist = m3_history(blks)
    short = [h for h, b in zip(hist, blks) if b["N"] == N and h[0] == 0]
    assert any(h[1] == 0 and h[2] >= 4 for h in short)                 # a run of impulse blocks: lW_no >= 4
    assert any(h[1] == 0 and h[2] < 4 for h in short)
    assert any(h[1] != 0 for h in short)                               # an impulse block after another kind
    assert any(h[3] for h in short)                                    # impulse, padding, impulse: impadnum set


def test_click_trains_at_8k_is_n256_without_m3(oracle):
    blks = blocks(oracle, "click_trains_1ch_8000_q0.5")
    assert {b["N"] for b in blks} == {512} and {b["block_mode"] for b in blks} == {0, 1}
    assert entry("click_trains_1ch_8000_q0.5")["rate"] < 26000         # set_m3p: hs_rate clear


def test_gated_bands_silence_the_magnitude_channel_alone(oracle):
    blks = blocks(oracle, "gated_bands_2ch_44100_q0.5")
    # post_valid is nonzero[] as floor1_encode returns it, before couple/quantise sets both flags of a live pair
    one = [b for b in blks if b["post_valid"][0] == 0 and b["post_valid"][1] == 1]
    assert one and all(b["nonzero"].tolist() == [1, 1] for b in one)
    assert any(b["post_valid"].tolist() == [0, 0] for b in blks)       # both flags clear
    blks = blocks(oracle, "gated_bands_6ch_48000_q0.1")
    assert any(0 < b["post_valid"][:5].sum() < 5 for b in blks)


def test_overdriven_noise_leaves_the_floor_range(oracle):
    blks = blocks(oracle, "overdriven_noise_2ch_44100_q-0.1")
    assert any(((b["post"][c] & 0x7fff) == 1023).any() for b in blks for c in range(2) if b["post_valid"][c])


def test_faint_and_zero_signals(oracle):
    blks = blocks(oracle, "faint_noise_2ch_44100_q0.5")
    assert {0, 1, 2, 3} <= {b["block_mode"] for b in blks}
    # whole spectra below -140 dB, the offset of the first bark-noise pass, in long and in short blocks; then floors
    for modes in ((3,), (0, 1)):
        assert any(b["block_mode"] in modes and b["logmdct"].max() < -140 and not b["post_valid"].any() for b in blks)
    assert any(b["post_valid"].all() and np.abs(b["pcm"]).max() < 2e-5 for b in blks)
    blks = blocks(oracle, "zero_tail_2ch_44100_q0.5")
    assert not blks[0]["post_valid"].any() and not blks[-1]["post_valid"].any() and blks[-1]["eos"]
    assert any(b["post_valid"].all() for b in blks)


def test_managed_witnesses(oracle):
    # faint noise at b256000: a block whose channels have a floor at the middle rate (packetblob 7) while the blobs at
    # both ends hold nothing but the header and two "floor unused" bits
    blks = blocks(oracle, "faint_noise_2ch_44100_b256000")
    assert any(b["post_valid"].all() and b["blob_bytes"][0] == 1 and b["blob_bytes"][14] == 1 and b["blob_bytes"][7] > 4
               for b in blks)
    # overdriven noise under a maximum rate: blob 0 is chosen and the packet handed out is shorter than that blob was
    blks = blocks(oracle, "overdriven_noise_2ch_44100_b128000_max144000_min112000")
    cut = [b for b in blks if len(b["packet"]) < b["blob_bytes"][b["choice"]]]
    assert len(cut) >= 3 and all(b["choice"] == 0 for b in cut)


# ---- the tool ---------------------------------------------------------------------------------------------------------
def design_rows():
    """(target name, classification) of the rows of DESIGN.md's table that name a target"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = text.index("Oracle branches: which ones the tests reach")
    rows = re.findall(r"^\|[^|\n]*\|[^|\n]*\| *`([a-z0-9_]+)` *\| *([^|\n]+?) *\|", text[at:], flags=re.M)
    assert rows
    return rows


def test_tool_counts_every_target_the_design_table_calls_reached():
    r = oracle_reach.measure("reach")
    assert r["blocks"] > 1000
    known = oracle_reach.targets()
    rows = design_rows()
    reached = [name for name, cls in rows if cls.startswith("reached by")]
    assert len(reached) >= 8
    for name, cls in rows:
        assert name in known, f"DESIGN.md names the target {name}, oracle/*.c has no such tag"
        if cls.startswith("reached by"):
            assert r["targets"][name]["count"] > 0, f"{name}: {cls}, but the reach corpus never executes it"
        else:
            assert r["targets"][name]["count"] == 0, f"{name}: {cls}, but the reach corpus executes it"
    for name in ("poste_positive", "poste_below_tenth", "postecho_npeak_minus1", "m8_skip_postecho"):
        assert name in reached


def _suite_slice(args):
    so, index, count = args
    o = orc.Oracle(so)
    hits = []
    for e in oracle_reach.suite_corpus()[index::count]:
        seq = walk(o, e["ch"], e["rate"], e["q"], e["bitrate"], e["make"](), chunk=None if e.get("one_write") else 1024,
                   finish=e.get("eos", True), capture=False)
        last = 0
        for b in seq:
            for c in range(e["ch"]):
                ret, raw, _ = detector(b["pcm"][c], b["block_mode"], last)
                assert ret == b["poste"][c]
                if raw is not None:
                    hits.append((e["name"], float(ret), float(raw)))
            last = b["block_mode"]
    return hits


def test_the_suite_signals_do_not_reach_the_post_echo_arm(oracle):
    """Over everything the parity tests feed the encoder, the detector's difference is positive in ONE block: the
    windowed sine at 2ch 44100 q-0.1 (blocks of 4096), both channels far above the clamp.  No synth_signal or
    burst_signal stream gets there, no value lies below 30, none in (0, 0.1), and no block has it in one channel only."""
    so = oracle.lib._name
    jobs = max(1, min(8, os.cpu_count() or 1))
    with multiprocessing.get_context("fork").Pool(jobs) as pool:
        hits = [h for part in pool.map(_suite_slice, [(so, i, 4 * jobs) for i in range(4 * jobs)]) for h in part]
    assert sorted(h[0] for h in hits) == ["sine_2ch_44100_q-0.1"] * 2, hits
    assert all(h[1] >= 30 for h in hits), hits
