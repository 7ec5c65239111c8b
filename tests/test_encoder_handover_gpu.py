"""Three hand-overs of the encoder's workspace slots that applications reach and no other suite does.

profile_switch: device-built rounds go from graphs to plain launches (stage timing on) and back, with work of the other
form still in flight.  reset_in_flight: reset() with rounds pending, then the same objects encode from packet 0.
batch_after_rounds: vbm_analysis_batch2 entered while deferred rounds are pending on the internal streams.
Sizes, signals and the delay points are those of tests/test_ordering_gpu.py (tests/encode_calls.py)."""
import math

import numpy as np
import pytest
import torch

from tests.encode_calls import (CH, K, Q, RATE, S, check_oracle, delay, drain_host, make_setup,  # noqa: F401
                                signals)
from tests.gpuutil import TwinLedger

pytestmark = pytest.mark.gpu

NCHUNKS, PERIOD = 18, 12000


def chunk(base, c):
    return base[:, :, c * 1024:(c + 1) * 1024].repeat(S // K, 1, 1).contiguous()


def device_encoder(v, monkeypatch):
    monkeypatch.setenv("VBM_WORKSPACES", "4")
    setup = make_setup(v, None)
    enc = v.Encoder(setup, S, max_batch=v.lib.vbm_device_round_lanes(setup._h, S))
    return enc, v.FrontEnd(enc)


def device_schedule(cuda, enc, fe, base, before=None, after=None):
    """the 18 writes of run_device_rounds (tests/encode_calls.py) (lazy=2, a consumer stream); before / after: {write: call}"""
    led = TwinLedger(S, K, cuda)
    consumer = torch.cuda.Stream(device=cuda)
    for c in range(NCHUNKS):
        if before and c in before:
            before[c]()
        fe.write(chunk(base, c))
        info, packets, nbytes, counts = fe.encode_rounds_device(nrounds=2, lazy=2)
        fe.join(consumer)
        with torch.cuda.stream(consumer):
            led.add_device_rounds(info, packets, nbytes, f"write {c}")
        consumer.synchronize()
        if after and c in after:
            after[c]()
    fe.device_stats()
    assert fe.refused_writes == 0
    torch.cuda.synchronize()
    drain_host(fe, led, "drain")
    fe.finish()
    drain_host(fe, led, "end of stream")
    led.finish("device-built rounds")
    return led


def host_schedule(cuda, fe, base):
    led = TwinLedger(S, K, cuda)
    for c in range(NCHUNKS):
        fe.write(chunk(base, c))
        drain_host(fe, led, f"write {c}")
    fe.finish()
    drain_host(fe, led, "end of stream")
    led.finish("host-built rounds")
    return led


@pytest.mark.parametrize("point", ["none", "dev_big_back", "job_back"])
def test_profile_switch(oracle, cuda, monkeypatch, delay, point):
    """writes 0-6 as graphs (plain launch, capture and replays of all four workspaces), 7-10 as plain launches on the job
    streams with stage timing, the rest as graphs again"""
    import vorbis_aotuv_lancer_amd as v
    if point != "none":
        delay(point)
    base = torch.from_numpy(np.stack(signals(NCHUNKS, PERIOD))).to(cuda)
    enc, fe = device_encoder(v, monkeypatch)
    prof = {}

    def end():
        prof["ms"], prof["calls"] = enc.profile_end()

    led = device_schedule(cuda, enc, fe, base, before={7: lambda: enc.profile_begin(4)}, after={10: end})
    check_oracle(led, oracle, NCHUNKS, PERIOD)
    assert prof["calls"] >= 1, prof
    names = [v.lib.vbm_encoder_stage_name(k).decode() for k in range(v.lib.vbm_encoder_stage_count())]
    for k, name in enumerate(names):
        ms = prof["ms"][name]
        assert math.isfinite(ms) and ms >= 0, (name, ms)
        if k != 2:      # (stage 2, "transpose", is retired: nothing launches it)
            assert ms > 0, (name, ms)
    fe.close()
    enc.close()


@pytest.mark.parametrize("form", ["device", "host"])
def test_reset_in_flight(oracle, cuda, monkeypatch, form):
    """six writes with nothing joined, reset of front end and encoder, then the whole schedule on the same objects"""
    import vorbis_aotuv_lancer_amd as v
    base = torch.from_numpy(np.stack(signals(NCHUNKS, PERIOD))).to(cuda)
    if form == "device":
        enc, fe = device_encoder(v, monkeypatch)
    else:
        enc = v.Encoder(make_setup(v, None), S)
        fe = v.FrontEnd(enc)
    for c in range(6):
        fe.write(chunk(base, c))
        if form == "device":
            fe.encode_rounds_device(nrounds=2, lazy=2)
        else:
            while fe.encode_rounds(min_rounds=64, max_rounds=4, lazy=True)[3]:
                pass
    fe.reset()          # (the front end's reset leaves the encoder's carried state alone)
    enc.reset()
    led = device_schedule(cuda, enc, fe, base) if form == "device" else host_schedule(cuda, fe, base)
    check_oracle(led, oracle, NCHUNKS, PERIOD)
    fe.close()
    enc.close()


@pytest.mark.parametrize("two", [False, True], ids=["one_stream", "two_stream"])
def test_batch_after_rounds(cuda, delay, two):
    """vbm_analysis_batch2 for every stream right behind deferred host-built rounds whose back halves are held up, against
    the same call on an encoder that went through the same rounds and was joined and idle before it"""
    import vorbis_aotuv_lancer_amd as v
    base = torch.from_numpy(np.stack(signals(NCHUNKS, PERIOD))).to(cuda)
    g = torch.Generator(device=cuda).manual_seed(3)
    blocks = (0.4 * (torch.rand((S, CH, 2048), generator=g, device=cuda) - 0.5)).contiguous()
    ids = np.arange(S, dtype=np.int32)
    fl = np.full(S, 3, np.uint8)
    setup = v.Setup(CH, RATE, Q)
    res = []
    for pending in (True, False):
        delay(*(["job_back"] if pending else []))
        enc = v.Encoder(setup, S)
        fe = v.FrontEnd(enc)
        nblocks = 0
        for c in range(8):
            fe.write(chunk(base, c))
            while True:
                counts = fe.encode_rounds(min_rounds=64, max_rounds=4, lazy=pending)[3]
                if not counts:
                    break
                nblocks += sum(counts)
        assert nblocks >= 4 * S, nblocks
        if not pending:
            fe.join()
            torch.cuda.synchronize()
        back = torch.cuda.Stream(device=cuda) if two else None
        out = (torch.empty((S, enc.max_packet_bytes), dtype=torch.uint8, device=cuda),
               torch.empty((S,), dtype=torch.int32, device=cuda))
        enc.analysis_batch(3, ids, fl, blocks, back_stream=back, out=out)
        torch.cuda.synchronize()
        res.append(out)
        fe.close()
        enc.close()
    assert bool((res[0][1] == res[1][1]).all()) and bool((res[0][1] > 0).all())
    assert bool((res[0][0] == res[1][0]).all()), "packets differ with rounds pending at the call's entry"
