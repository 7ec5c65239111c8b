"""k_couple_fast with its constants handed over by the host (vbm_batch.cc): quantised residue and packets against the
oracle, at the batch sizes and in the setups that pick its variants.

  batch sizes  1, 9 and 65 stream-blocks of long blocks, all streams in one batch (tests/stage_shapes.py).  A workgroup
               takes 8 columns: a lone column, a tail workgroup of one, and a second 64-lane tile with a tail
  stereo q5    one coupling step: both channels of a stream-block in a lane (MODE 1); constants of blob PACKETBLOBS/2
  mono q5      no coupling: a column is a channel-block (MODE 0)
  2ch 128 kb/s managed: the kernel walks all fifteen packetblobs, each with its own entry of the constants (point limit,
               pre / post point amplitudes, sliding lowpass).  Every blob's packet is compared, which pins every entry;
               the stage `residue` holds one blob's values only and is left to the VBR cases.

The signals are those of tests/test_tonemask_shapes_gpu.py (silence with clicks, a full-scale sine, noise stepping
up, two close tones; stereo channels differ), which give residues on both sides of the point-stereo limits."""
import pytest

from tests import stage_shapes as ss
from tests.test_tonemask_shapes_gpu import KINDS, shape_signal

SIZES = [1, 9, 65]
SETUPS = [(2, 0.5, None), (1, 0.5, None), (2, None, 128000)]
DISTINCT = 8
_cache = {}


def distinct_streams(oracle, ch, q, bitrate):
    key = (ch, q, bitrate)
    if key not in _cache:
        keep = ("lW", "nW", "block_mode", "pcm", "packet") + (("blobs", "blob_bytes", "choice") if bitrate else ("residue",))
        _cache[key] = [ss.oracle_stream_blocks(oracle, ch, 44100, q, shape_signal(KINDS[d % 4], d // 4, ch, 44100),
                                               bitrate=bitrate, keep=keep) for d in range(DISTINCT)]
    return _cache[key]


def streams_for(oracle, ch, q, bitrate, B):
    d = distinct_streams(oracle, ch, q, bitrate)
    return [d[(s + 2) % DISTINCT] for s in range(B)]        # (a lone stream: the noise signal)


@pytest.mark.parametrize("ch,q,bitrate", SETUPS)
def test_oracle_long_blocks_meet_in_one_batch(oracle, ch, q, bitrate):
    """(CPU) at every size some call holds a long block of every stream"""
    for B in SIZES:
        calls = ss.schedule(streams_for(oracle, ch, q, bitrate, B))
        assert 3 in ss.full_batches(calls, B), B


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("ch,q,bitrate", SETUPS)
def test_residue_and_packets_at_batch_size(oracle, cuda, ch, q, bitrate, B):
    import vorbis_aotuv_lancer_amd as v
    streams = streams_for(oracle, ch, q, bitrate, B)
    calls = ss.schedule(streams)
    assert 3 in ss.full_batches(calls, B)
    setup = v.Setup(ch, 44100, q, bitrate=bitrate)
    enc = v.Encoder(setup, B)

    def blobs(k, mode, ids, blks, bad):
        choice = enc.fetch("choice").cpu().numpy()
        for kb in range(15):
            bp, bn = enc.fetch_blob(kb)
            bp, bn = bp.cpu().numpy(), bn.cpu().numpy()
            for i, b in enumerate(blks):
                if bn[i] != b["blob_bytes"][kb] or bytes(bp[i, :max(bn[i], 0)]) != b["blobs"][kb]:
                    bad.append((k, mode, len(ids), "blob", (ids[i], kb, int(bn[i]), b["blob_bytes"][kb])))
        for i, b in enumerate(blks):
            if choice[i] != b["choice"]:
                bad.append((k, mode, len(ids), "choice", (ids[i], int(choice[i]), b["choice"])))

    try:
        bad = ss.run_schedule(enc, cuda, streams, calls, () if bitrate else ("residue",), on_batch=blobs if bitrate else None)
        assert not bad, bad[:8]
    finally:
        enc.close()
        setup.close()
