"""Full device pipeline vs the oracle: stage by stage and packet by packet.

NS independent streams are encoded by the oracle on the CPU (block sequence, raw block PCM,
every captured stage vector, packets).  The same blocks are then pushed through
vbm_analysis_batch in lock-step (k-th block of every stream per step, grouped by block type),
and every intermediate the C ABI exposes is compared bit-for-bit."""
import pytest
import torch

from tests.encode_calls import run_lockstep
from tests.encode_oracle import walk
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu

STAGES_F = ["mdct_raw", "logfft", "logmdct", "noise", "tone", "logmask", "mdct"]
STAGES_I = ["post_valid", "residue", "nonzero"]


def oracle_blocks(oracle, ch, rate, q, seconds, seed):
    """1024 samples per write, the end of the stream not declared"""
    sig = synth_signal(ch, rate, int(seconds * rate), seed=seed, level=1.0 if seed % 3 else 0.05)
    return walk(oracle, ch, rate, q, pcm=sig, finish=False)


def run_case(oracle, cuda, ch, rate, q, nstreams, seconds, check_stages=True, res1_channels=(), sub_batches=1,
             two_streams=False):
    import vorbis_aotuv_lancer_amd as v
    streams = [oracle_blocks(oracle, ch, rate, q, seconds, seed=100 + s) for s in range(nstreams)]
    nsteps = min(len(b) for b in streams)
    assert nsteps > 20
    setup = v.Setup(ch, rate, q)
    enc = v.Encoder(setup, nstreams)
    enc.set_sub_batches(sub_batches)
    assert enc.sub_batches == sub_batches
    # two_streams: vbm_analysis_batch2, back half on its own stream; no host sync between the calls
    stat = run_lockstep(enc, cuda, streams, ch, STAGES_F if check_stages else (), STAGES_I if check_stages else (),
                        res1_channels, stop="shortest", back_stream=torch.cuda.Stream(device=cuda) if two_streams else None)
    enc.close()
    setup.close()
    return stat["modes"], nsteps


def test_stereo_q5_stage_and_packet_parity(oracle, cuda):
    modes, nsteps = run_case(oracle, cuda, 2, 44100, 0.5, nstreams=24, seconds=4.0)
    assert modes == {0, 1, 2, 3}     # impulse, padding, transition and long blocks all occurred


def test_stereo_q1_packet_parity(oracle, cuda):
    # q0.1: live noise normalisation (normal_start 16/128) and the 128x4 short floor
    run_case(oracle, cuda, 2, 44100, 0.1, nstreams=8, seconds=3.0)


def test_surround_51_q8_packet_parity(oracle, cuda):
    # 6 channels, two submaps: 5-channel res-2 (uncoupled) + LFE res-1
    run_case(oracle, cuda, 6, 48000, 0.8, nstreams=6, seconds=3.0, res1_channels=(5,))


def test_stereo_q5_many_streams_in_sub_batches(oracle, cuda):
    """150 streams = 3 tiles of 64 stream-blocks, encoded as 2 slices on separate internal HIP streams
    (vbm_encoder_set_sub_batches): packets must still equal the oracle's for every stream."""
    run_case(oracle, cuda, 2, 44100, 0.5, nstreams=150, seconds=0.7, check_stages=False, sub_batches=2)


def test_stereo_q5_two_stream_form(oracle, cuda):
    """vbm_analysis_batch2: back half (floor, couple/quantise, packets) of every call on a second stream,
    overlapping the front half of the next call, no host synchronisation in between; all block types."""
    modes, _ = run_case(oracle, cuda, 2, 44100, 0.5, nstreams=20, seconds=3.0, check_stages=False, two_streams=True)
    assert modes == {0, 1, 2, 3}


def test_two_stream_form_with_sub_batches(oracle, cuda):
    """two-stream form + sub-batches: the back half of a call runs as two slices (caller's back stream and an
    internal one beside it), joined before the workspace is handed back"""
    run_case(oracle, cuda, 2, 44100, 0.5, nstreams=150, seconds=0.7, check_stages=False, sub_batches=2, two_streams=True)
