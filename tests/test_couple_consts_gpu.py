"""k_couple_fast with its constants handed over by the host (vbm_batch.cc): quantised residue and packets against the
oracle, at the batch sizes and in the setups that pick its variants.

  batch sizes  1, 9 and 65 stream-blocks of long blocks, all streams in one batch (tests/stage_shapes.py).  A workgroup
               takes 8 columns: a lone column, a tail workgroup of one, and a second 64-lane tile with a tail
  stereo q5    one coupling step: both channels of a stream-block in a lane (MODE 1); constants of blob PACKETBLOBS/2
  mono q5      no coupling: a column is a channel-block (MODE 0)
  2ch 128 kb/s managed: the kernel walks all fifteen packetblobs, each with its own entry of the constants (point limit,
               pre / post point amplitudes, sliding lowpass).  Every blob's packet is compared, which pins every entry;
               the stage `residue` holds one blob's values only and is left to the VBR cases.

The signals are those of tests/test_tonemask_shapes_gpu.py (shape_signal of tests/encode_oracle.py: silence with clicks,
a full-scale sine, noise stepping up, two close tones; stereo channels differ), which give residues on both sides of the
point-stereo limits."""
import pytest

from tests import stage_shapes as ss
from tests.encode_calls import fetch_blobs
from tests.encode_oracle import compare_blobs, streams_for

SIZES = [1, 9, 65]
SETUPS = [(2, 0.5, None), (1, 0.5, None), (2, None, 128000)]


def streams(oracle, ch, q, bitrate, B):
    keep = ("lW", "nW", "block_mode", "pcm", "packet") + (("blobs", "blob_bytes", "choice") if bitrate else ("residue",))
    return streams_for(oracle, ch, 44100, q, B, keep, distinct=8, first=2, bitrate=bitrate)    # (a lone stream: the noise signal)


@pytest.mark.parametrize("ch,q,bitrate", SETUPS)
def test_oracle_long_blocks_meet_in_one_batch(oracle, ch, q, bitrate):
    """(CPU) at every size some call holds a long block of every stream"""
    for B in SIZES:
        calls = ss.schedule(streams(oracle, ch, q, bitrate, B))
        assert 3 in ss.full_batches(calls, B), B


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("ch,q,bitrate", SETUPS)
def test_residue_and_packets_at_batch_size(oracle, cuda, ch, q, bitrate, B):
    import vorbis_aotuv_lancer_amd as v
    blocks = streams(oracle, ch, q, bitrate, B)
    calls = ss.schedule(blocks)
    assert 3 in ss.full_batches(calls, B)
    setup = v.Setup(ch, 44100, q, bitrate=bitrate)
    enc = v.Encoder(setup, B)

    def blobs(call):
        compare_blobs(fetch_blobs(enc), enc.fetch("choice").cpu().numpy(), call.blks, call.label)

    try:
        ss.run_schedule(enc, cuda, blocks, calls, () if bitrate else ("residue",), ch, on_call=blobs if bitrate else None)
    finally:
        enc.close()
        setup.close()
