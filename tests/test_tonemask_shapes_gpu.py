"""k_tonemask at the batch sizes, row lengths and signals where its chase and fill phases can go wrong: the stage
output `tone` (and the packets) of every batch, bit for bit against the oracle.

Batch sizes: B = 1, 7, 8, 9 and 65 streams side by side (tests/stage_shapes.py: every block type is met at least once
by all B streams in one batch).  A workgroup takes 8 channel-blocks and a tile 64: mono batches are 1, 7, 8, 9 and 65
channel-blocks (a lone block, a tail workgroup of 7 and of 1, a full workgroup, a second tile); a stereo batch has two
channel-blocks per stream, so the same stream counts give 2, 14, 16, 18 and 130.

Seed rows: total_octave_lines = 64 * octaves + 9, so the last 64-line chunk of a row always holds 9 lines.  Short
blocks of 256 samples have the fewest of any shipped class (585), long blocks of 4096 the most (841: only 2ch 44100
q-0.1 has them, with 649 for its 512-sample short blocks); mono classes go up to 777 (2048 samples).

Signals (all start with silence, begin at one sample and have a burst at another, so all four block types occur twice
and the streams meet at them):
  silence   digital silence with two clicks in channel 0: before and round a click every seed of a row is equal, the
            walk pops on ties everywhere; the other channel of a stereo stream stays silent throughout
  sine      one full-scale sine switched on: long monotone flanks, few survivors
  noise     white noise, faint and then loud: survivors every few lines, so in the last seven lines of a chunk and
            the first of the next, where the walk's result is handed to the left neighbour
  twotone   two tones an eighth of an octave (8 seed lines = the walk's reach) apart, of equal and of unequal level
Streams beyond the first four take the same four kinds at other levels and frequencies (16 distinct streams).  The
signals are shape_signal of tests/encode_oracle.py."""
import pytest

from tests import stage_shapes as ss
from tests.encode_oracle import KINDS, distinct_streams, streams_for

CLASSES = [(1, 44100, 0.5), (2, 44100, 0.5), (2, 44100, -0.1)]
SIZES = [1, 7, 8, 9, 65]
SHARED = dict(keep=("lW", "nW", "block_mode", "pcm", "packet", "tone"), distinct=16)


@pytest.mark.parametrize("ch,rate,q", CLASSES)
def test_oracle_signals_reach_every_block_type_together(oracle, ch, rate, q):
    """(CPU) what the GPU cases below rely on: at every size all four block types occur in a batch of all B streams,
    and the silent blocks are there: rows whose seeds are all equal."""
    for B in SIZES:
        streams = streams_for(oracle, ch, rate, q, B, **SHARED)
        assert ss.full_batches(ss.schedule(streams), B) == {0, 1, 2, 3}, B
    for first in range(4):      # a lone stream of each kind
        one = streams_for(oracle, ch, rate, q, 1, first=first, **SHARED)
        assert ss.full_batches(ss.schedule(one), 1) == {0, 1, 2, 3}, KINDS[first]
    silent = {b["block_mode"] for b in distinct_streams(oracle, ch, rate, q, **SHARED)[0] if not b["pcm"].any()}
    assert {1, 3} <= silent, silent     # all-zero padding and long blocks


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("ch,rate,q", CLASSES)
def test_tone_stage_at_batch_size(oracle, cuda, ch, rate, q, B):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(ch, rate, q)
    firsts = range(4) if B == 1 else (0,)       # a lone block of every kind
    try:
        for first in firsts:
            streams = streams_for(oracle, ch, rate, q, B, first=first, **SHARED)
            calls = ss.schedule(streams)
            assert ss.full_batches(calls, B) == {0, 1, 2, 3}
            enc = v.Encoder(setup, B)
            try:
                ss.run_schedule(enc, cuda, streams, calls, ("tone",), ch)
            finally:
                enc.close()
    finally:
        setup.close()
