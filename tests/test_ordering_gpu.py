"""Ordering of the internal HIP streams, made adversarial on purpose.

The encode path runs on several internal HIP streams (front end, one per block type, front / back half of the big
batch, HIP graphs per workspace); events order them.  A missing edge normally shows once in many runs.  Here every
marked point of the host code (csrc/vbm_internal.h, enum vbm_delay_point) gets, one point per case, a kernel that
spins for milliseconds in front of the work behind it (vbm_debug_set_delay): whatever is not ordered behind the
delayed work runs ahead of it, deterministically.  Packets may not change: every stream against its twin and the
distinct signals against the oracle, for the host-built rounds, the device-built (graph) rounds and the two-stream
per-block form.  A second family of cases fills every scratch buffer with 0xFF between calls
(vbm_debug_poison_*): nothing a batch reads may be left over from the batch that used the workspace before.
The sizes, signals, rounds runners and the `delay` fixture are those of tests/encode_calls.py."""
import numpy as np
import pytest
import torch

from tests.encode_calls import (CH, MANAGED, Q, RATE, S, check_oracle, delay, run_device_rounds,  # noqa: F401 (delay: fixture)
                                run_host_rounds)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("point", ["none", "job_big", "job_small", "job_state", "job_back", "job_out", "fe_fork", "fe_shift",
                                   "fe_write"])
def test_host_built_rounds_with_delays(oracle, cuda, delay, point):
    nchunks, period = 10, 6000
    if point != "none":
        delay(point)
    check_oracle(run_host_rounds(cuda, nchunks, period), oracle, nchunks, period)


def test_host_built_rounds_deferred_joins_with_delays(oracle, cuda, delay):
    """several rounds in flight (vbm_frontend_encode_rounds) with the small batches and every back half held up"""
    nchunks, period = 10, 6000
    delay("job_small", "job_back")
    check_oracle(run_host_rounds(cuda, nchunks, period, multi=True), oracle, nchunks, period)


@pytest.mark.parametrize("point", ["none", "dev_big_front", "dev_big_back", "dev_small_front", "dev_small_back", "dev_plan",
                                   "dev_out", "fe_shift", "fe_write"])
def test_device_built_rounds_with_delays(oracle, cuda, monkeypatch, delay, point):
    nchunks, period = 18, 12000
    if point != "none":
        delay(point)
    check_oracle(run_device_rounds(cuda, monkeypatch, nchunks, period), oracle, nchunks, period)


@pytest.mark.parametrize("point", ["none", "job_back", "job_small", "job_out", "job_state"])
def test_managed_host_built_rounds_with_delays(oracle, cuda, delay, point):
    """Managed bitrate: the front half and the fifteen packetblobs of a batch run beside the back halves of the batches
    before it; the bitrate manager's choice (reservoirs: state carried from block to block, lib/bitrate.c:98-226) is the
    step that waits for them.  A stream changes block type — and with it the internal HIP stream — at every burst; with
    the back half of a batch held up, a choice that did not wait would see reservoirs one block old.  (Tried and not kept: a
    case that switches the wait off and expects different packets — the reservoirs' sums do not depend on the order of the
    additions, so a mis-ordered choice only shows when it flips a choice, which a third of a second of audio does not do.)"""
    nchunks, period = 10, 6000
    if point != "none":
        delay(point)
    check_oracle(run_host_rounds(cuda, nchunks, period, bitrate=MANAGED), oracle, nchunks, period, MANAGED)


@pytest.mark.parametrize("point", ["none", "job_back", "job_big", "job_out"])
def test_managed_device_built_rounds_with_delays(oracle, cuda, monkeypatch, delay, point):
    nchunks, period = 12, 6000
    if point != "none":
        delay(point)
    check_oracle(run_device_rounds(cuda, monkeypatch, nchunks, period, bitrate=MANAGED), oracle, nchunks, period, MANAGED)


def test_host_built_rounds_poisoned_scratch(oracle, cuda):
    nchunks, period = 10, 6000
    check_oracle(run_host_rounds(cuda, nchunks, period, poison=True), oracle, nchunks, period)


def test_device_built_rounds_poisoned_scratch(oracle, cuda, monkeypatch):
    nchunks, period = 18, 12000
    check_oracle(run_device_rounds(cuda, monkeypatch, nchunks, period, poison=True), oracle, nchunks, period)


@pytest.mark.parametrize("point", ["batch_front", "batch_back"])
def test_two_stream_form_with_delays(cuda, delay, point):
    """vbm_analysis_batch2 (front half and back half on two streams, workspaces alternating): six calls, one half held
    up at every call, against the one-stream form without delays"""
    import vorbis_aotuv_lancer_amd as v
    g = torch.Generator(device=cuda).manual_seed(3)
    setup = v.Setup(CH, RATE, Q)
    ids = np.arange(S, dtype=np.int32)
    fl = np.full(S, 3, np.uint8)
    blocks = [(0.4 * (torch.rand((S, CH, 2048), generator=g, device=cuda) - 0.5)).contiguous() for _ in range(6)]
    res = []
    for two in (False, True):
        if two:
            delay(point)
        enc = v.Encoder(setup, S)
        back = torch.cuda.Stream(device=cuda) if two else None
        outs = [(torch.empty((S, enc.max_packet_bytes), dtype=torch.uint8, device=cuda),
                 torch.empty((S,), dtype=torch.int32, device=cuda)) for _ in range(6)]
        for k in range(6):
            enc.analysis_batch(3, ids, fl, blocks[k], back_stream=back, out=outs[k])
        torch.cuda.synchronize()
        res.append(outs)
        enc.close()
    for k in range(6):
        assert bool((res[0][k][1] == res[1][k][1]).all()) and bool((res[0][k][1] > 0).all())
        assert bool((res[0][k][0] == res[1][k][0]).all()), f"call {k}: packets differ with {point} held up"
