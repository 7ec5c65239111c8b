"""The correlated-channel corpus (tests/image_signals.py) has teeth — conditions on the oracle's own output, no GPU.

Rows of `residue` are channels; of a coupling step (magnitude channel, angle channel) of the setup, the angle row is
what the step left in its angle channel.  A channel can serve in several steps (coupled 5.1: (0, 2), (3, 4), (0, 1),
(0, 3)): the capture holds every row as the LAST step left it, so a step is judged on its rows only where no later
step rewrites one of them as its angle (`judged_steps`).

The tie witnesses, per stream: non-zero magnitude values, non-zero angle values, and angle values equal to
-2 |magnitude| at the same bin.  The one input of the suite that was the same in every channel before this corpus, the
reference's windowed sine (tests/test_reference_input_gpu.py: eleven blocks at 2ch 44100 q0.5), has 239 non-zero
magnitude values in its whole stream; the smallest dual-mono stream here has 15569."""
import numpy as np
import pytest

from tests.image_cases import (DECODED, DECODED_IDS, blocks, check_relation, cid, encode, independent, model_spectra,
                               twins)
from tests.image_signals import IMAGES, LADDER, class_of, classes, coupling_steps, images_of, seconds_of

STEREO = [c for c in classes() if c[0] == 2]
COUPLED_6 = [c for c in classes() if c[0] == 6 and coupling_steps(*c)]
MANAGED_STEREO = [c for c in STEREO if c[3] is not None]


def witnesses(blks, mag, ang):
    """(non-zero magnitude values, non-zero angle values, angle values of -2 |magnitude|) over the stream"""
    nm = sum(int((b["residue"][mag] != 0).sum()) for b in blks)
    na = sum(int((b["residue"][ang] != 0).sum()) for b in blks)
    n2 = sum(int(((b["residue"][ang] != 0) & (b["residue"][ang] == -2 * np.abs(b["residue"][mag]))).sum()) for b in blks)
    return nm, na, n2


def judged_steps(steps):
    """the steps neither of whose rows a later step rewrites as its angle row"""
    return [(m, a) for k, (m, a) in enumerate(steps) if not {m, a} & {a2 for _, a2 in steps[k + 1:]}]


def test_every_stream_of_the_corpus_has_all_four_block_types(oracle):
    assert len(IMAGES) >= 60
    for e in IMAGES:
        blks = encode(oracle, e["name"], class_of(e), e["make"])
        assert {b["block_mode"] for b in blks} == {0, 1, 2, 3}, e["name"]
        assert blks[-1]["eos"] and not (blks[0]["poste"] > 0).any()


def test_every_stereo_class_has_the_ladder():
    assert len(STEREO) == 8
    for c in STEREO:
        names = [e["name"] for e in images_of(*c)]
        assert all(any(n.startswith(x + "_2ch") for n in names) for x in LADDER), c
        assert coupling_steps(*c) == [(0, 1)]


@pytest.mark.parametrize("c", STEREO, ids=cid)
def test_dual_mono_is_tied_in_every_bin(oracle, c):
    blks = blocks(oracle, c, "dual_mono")
    for k, b in enumerate(blks):
        assert np.array_equal(b["mdct"][0].view(np.uint32), b["mdct"][1].view(np.uint32)), k
        assert not b["residue"][1].any(), k
    nm, na, n2 = witnesses(blks, 0, 1)
    print(f"{cid(c)} dual_mono: {nm} / {na} / {n2}")
    assert nm >= 10000          # (the windowed sine of test_reference_input_gpu has 239)


@pytest.mark.parametrize("c", STEREO, ids=cid)
def test_inverted_angle_is_minus_twice_the_magnitude(oracle, c):
    blks = blocks(oracle, c, "inverted")
    for k, b in enumerate(blks):
        mag, ang = b["residue"][0], b["residue"][1]
        live = ang != 0
        assert np.array_equal(ang[live], -2 * np.abs(mag[live])), k
    nm, na, n2 = witnesses(blks, 0, 1)
    print(f"{cid(c)} inverted: {nm} / {na} / {n2}")
    assert na == n2 >= 1000


@pytest.mark.parametrize("c", STEREO, ids=cid)
def test_near_mono_ladder(oracle, c):
    count = {x: witnesses(blocks(oracle, c, x), 0, 1) for x in ("dual_mono", "near_mono_40", "near_mono_80")}
    count["independent"] = witnesses(independent(oracle, c), 0, 1)
    print(f"{cid(c)}: " + ", ".join(f"{k} {v[0]} / {v[1]} / {v[2]}" for k, v in count.items()))
    assert 0 == count["dual_mono"][1] < count["near_mono_40"][1] < count["independent"][1]
    assert count["near_mono_80"][1] <= count["near_mono_40"][1]
    if c[1] == 44100 and c[2] in (0.1, 0.5, 1.0):
        assert count["near_mono_80"][1] > 0


@pytest.mark.parametrize("c", COUPLED_6, ids=cid)
def test_coupled_51_all_same(oracle, c):
    """every coupling step's angle row is zero; the magnitude row of every step that can be judged is not, and neither
    is the channel outside the coupling"""
    steps = coupling_steps(*c)
    assert len(steps) == 4 and len({a for _, a in steps}) == 4
    blks = blocks(oracle, c, "all_same")
    coupled = sorted({x for s in steps for x in s})
    for k, b in enumerate(blks):
        for x in coupled[1:]:
            assert np.array_equal(b["mdct"][coupled[0]].view(np.uint32), b["mdct"][x].view(np.uint32)), (k, x)
        for m, a in steps:
            assert not b["residue"][a].any(), (k, m, a)
    for m, a in judged_steps(steps):
        nm, na, n2 = witnesses(blks, m, a)
        print(f"{cid(c)} all_same step ({m}, {a}): {nm} / {na} / {n2}")
        assert nm >= 5000 * seconds_of(*c) and na == 0        # (10000 in 2 s, as for the stereo classes)
    rest = [x for x in range(c[0]) if x not in coupled]
    assert rest and all(any(b["residue"][x].any() for b in blks) for x in rest)


@pytest.mark.parametrize("c", COUPLED_6, ids=cid)
def test_coupled_51_alt_sign(oracle, c):
    """(M, -M, M, -M, M, -M): a step that pairs two even or two odd channels is tied like dual mono, one that pairs an
    even with an odd channel like the inverted pair.  The first judged step of opposite channels, (0, 1) in the shipped
    setups, has at least 1000 angle values of -2 |magnitude|."""
    steps = coupling_steps(*c)
    blks = blocks(oracle, c, "alt_sign")
    judged = judged_steps(steps)
    equal = [(m, a) for m, a in judged if (m - a) % 2 == 0]
    opposite = [(m, a) for m, a in judged if (m - a) % 2]
    assert equal and opposite
    for m, a in equal:
        assert witnesses(blks, m, a)[1] == 0, (m, a)
    nm, na, n2 = witnesses(blks, *opposite[0])
    print(f"{cid(c)} alt_sign step {opposite[0]}: {nm} / {na} / {n2}")
    assert n2 >= 1000


def test_managed_blob_choices(oracle):
    for c in MANAGED_STEREO:
        chosen = {}
        for x in ("dual_mono", "inverted"):
            blks = blocks(oracle, c, x)
            chosen[x] = {b["choice"] for b in blks}
            assert all(n > 0 for b in blks if b["post_valid"].any() for n in b["blob_bytes"]), (c, x)
        print(f"{cid(c)}: dual_mono chooses blobs {sorted(chosen['dual_mono'])}, inverted {sorted(chosen['inverted'])}")
        assert chosen["dual_mono"] != chosen["inverted"]


@pytest.mark.parametrize("c,image,kind", DECODED, ids=DECODED_IDS)
def test_decoded_spectra_are_copies_or_negatives(oracle, c, image, kind):
    """The model's spectrum of every packet: bit-identical rows for dual mono and for the coupled channels of 5.1
    all_same (channel 5 has a submap, and so a floor, of its own), rows that differ in the sign bit alone for the
    inverted pair wherever the pair was coupled losslessly."""
    _, blks, results = model_spectra(oracle, c, image)
    chans = twins(c)
    assert chans == ([0, 1] if c[0] == 2 else [0, 1, 2, 3, 4])
    assert all(r["status"] == 0 for r in results)
    neg, same = check_relation([r["spectrum"] for r in results], chans, kind, image)
    print(f"{cid(c)} {image}: {neg} bins exact negatives, {same} bit-identical")
