"""k_tonemask's chase phase (csrc/tone_chase.h: the two-mask step, speculative chunk starts, re-runs) with lanes that
re-run next to lanes that do not: the stage output `tone` and the packets of every batch, bit for bit against the oracle.

A workgroup takes eight channel-blocks and a wavefront the chase lanes of four of them.  The streams are the silent
ones with clicks (rows of equal seeds: every chunk's guessed start state is wrong, the re-runs cascade down the row) and
the noise ones (survivors every few lines, every guess right) of tests/test_tonemask_shapes_gpu.py's set, in turn.  In a
mono batch the channel-blocks of a workgroup then alternate between the two; in a stereo batch they go click channel,
silent channel, noise, noise.  Either way a wavefront holds lanes of both, so the re-run loop runs with part of the
wavefront switched off and the shuffles cross blocks that are in different rounds.

B = 1 is a lone block (of each of the two kinds), B = 9 a full workgroup and a tail workgroup of one or two blocks.  The
oracle's walks are those the shape tests already made (tests/encode_oracle.py keeps them for the session)."""
import pytest

from tests import stage_shapes as ss
from tests.encode_oracle import KINDS, distinct_streams

CLASSES = [(1, 44100, 0.5), (2, 44100, 0.5), (2, 44100, -0.1)]
SIZES = [1, 9]
SHARED = dict(keep=("lW", "nW", "block_mode", "pcm", "packet", "tone"), distinct=16)      # as test_tonemask_shapes_gpu.py
SILENCE, NOISE = KINDS.index("silence"), KINDS.index("noise")


def alternating(oracle, ch, rate, q, B, first):
    """B streams: silence and noise in turn (the variants of each kind one after the other), starting with kind `first`"""
    d = distinct_streams(oracle, ch, rate, q, **SHARED)
    order = [4 * (s // 2) + (first, SILENCE + NOISE - first)[s % 2] for s in range(8)]
    return [d[order[s % 8]] for s in range(B)]


@pytest.mark.parametrize("ch,rate,q", CLASSES)
def test_streams_alternate_and_meet(oracle, ch, rate, q):
    """(CPU) what the GPU cases rely on: the kinds alternate, all B streams go through every block type in one batch,
    and the silent streams have all-zero blocks (rows of equal seeds) of the padding and the long type"""
    for B in SIZES:
        for first in (SILENCE, NOISE):
            streams = alternating(oracle, ch, rate, q, B, first)
            assert ss.full_batches(ss.schedule(streams), B) == {0, 1, 2, 3}, (B, first)
    d = distinct_streams(oracle, ch, rate, q, **SHARED)
    nine = alternating(oracle, ch, rate, q, 9, SILENCE)
    assert all(nine[s] is d[4 * ((s % 8) // 2) + (SILENCE, NOISE)[s % 2]] for s in range(9))
    for s in (0, 2, 4, 6):
        assert {1, 3} <= {b["block_mode"] for b in nine[s] if not b["pcm"].any()}, s
    for s in (1, 3, 5, 7):
        assert all(b["pcm"].any() for b in nine[s][-4:]), s             # the noise is on to the end


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("ch,rate,q", CLASSES)
def test_tone_stage_with_mixed_reruns(oracle, cuda, ch, rate, q, B):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(ch, rate, q)
    try:
        for first in ((SILENCE, NOISE) if B == 1 else (SILENCE,)):
            streams = alternating(oracle, ch, rate, q, B, first)
            calls = ss.schedule(streams)
            assert ss.full_batches(calls, B) == {0, 1, 2, 3}
            enc = v.Encoder(setup, B)
            try:
                ss.run_schedule(enc, cuda, streams, calls, ("tone",), ch)
            finally:
                enc.close()
    finally:
        setup.close()
