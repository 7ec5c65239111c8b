"""The benchmarked flow with many calls in flight and no host wait, against the twins and the oracle.

bench.py's from-PCM leg enqueues write after write (resident PCM, rounds built on the device, lazy = 2, a consumer stream
joins after every call) and never waits: at any moment several calls are in flight across the workspaces and the output
ring.  Every other parity test of FrontEnd.encode_rounds_device blocks the host once per write (the twin ledger reads
back), so the deepest overlap they check is one call.  Here the window of tests/test_ordering_gpu.py's size (tests/encode_calls.py:
2048 stereo q5 streams, 8 twin signals) runs with nothing between the first write and the last that waits for the device: a
DeviceLog (tests/gpuutil.py) copies each call's outputs on the consumer's stream, the consumer releases the ring sets
(FrontEnd.release), and the ledger sees the log only after the window.  Right after the last call is enqueued the test
counts the calls whose consumer event has not completed: that is the depth the case reached, printed, and where a spin
kernel (vbm_debug_set_delay) makes the device slower than the host it must be at least 4, one more than the ring is deep.

The output ring's reuse guard (FrontEnd.release / the wait in encode_rounds_device) is what `slow_consumer` is about: the
consumer's stream is kept busy before every copy-out, the producer is not held up, so without the guard the producer
laps the consumer and the log holds packets of later calls."""
import numpy as np
import pytest
import torch

from tests import encode_calls as og
from tests.encode_calls import delay  # noqa: F401  (fixture)
from tests.gpuutil import DeviceLog, TwinLedger

pytestmark = pytest.mark.gpu

S, K, CH = og.S, og.K, og.CH
RING = 3                        # sets per round count (FrontEnd.encode_rounds_device)
CONSUMER_BUSY_MS = 3.0
_cache = {}


def bench_rounds(nchunks):
    """round counts of bench.py's default pattern, as tests/test_full_size_gpu.py::test_full_size_benchmarked_path"""
    return [3 if c < 6 else (2, 1, 1, 1)[c % 4] for c in range(nchunks)]


def spin_cycles(device, ms):
    """torch.cuda._sleep counts ticks of the device's clock: its rate, measured once before any window"""
    if "rate" not in _cache:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(100000)                       # (first use: module load)
        torch.cuda.synchronize(device)
        ticks = 2000000
        a.record()
        torch.cuda._sleep(ticks)
        b.record()
        torch.cuda.synchronize(device)
        _cache["rate"] = ticks / max(a.elapsed_time(b), 1e-3)          # ticks per millisecond
    return int(_cache["rate"] * ms)


def run_window(cuda, monkeypatch, oracle, nchunks, period, rounds, bitrate=None, workspaces="4", compact=False,
               consumer_busy=False):
    """-> (calls still in flight when the last one had been enqueued, the consumer's read-done events, the producer's events)"""
    import vorbis_aotuv_lancer_amd as v
    monkeypatch.setenv("VBM_WORKSPACES", workspaces)
    busy = spin_cycles(cuda, CONSUMER_BUSY_MS) if consumer_busy else 0
    base = torch.from_numpy(np.stack(og.signals(nchunks, period))).to(cuda)
    pcm = base.reshape(K, CH, nchunks, 1024).permute(2, 0, 1, 3).repeat(1, S // K, 1, 1).contiguous()   # [nchunks, S, ch, 1024]
    del base
    setup = og.make_setup(v, bitrate)
    enc = v.Encoder(setup, S, max_batch=v.lib.vbm_device_round_lanes(setup._h, S))
    fe = v.FrontEnd(enc)
    led = TwinLedger(S, K, cuda)
    consumer = torch.cuda.Stream(device=cuda)
    log = DeviceLog(fe, rounds, cuda, compact=compact)
    take = log.take_compact if compact else log.take
    read_done = [torch.cuda.Event(enable_timing=consumer_busy) for _ in range(nchunks)]
    released = [torch.cuda.Event() for _ in range(nchunks)]
    produced = [torch.cuda.Event(enable_timing=consumer_busy) for _ in range(nchunks)]
    torch.cuda.synchronize(cuda)
    # ---- the window: nothing in it waits for the device
    for c in range(nchunks):
        fe.write(pcm[c])
        out = fe.encode_rounds_device(nrounds=rounds[c], lazy=2)
        produced[c].record()             # the feeding stream is past the call, the guard's wait included
        fe.join(consumer)
        with torch.cuda.stream(consumer):
            if busy:
                torch.cuda._sleep(busy)
            take(c, *out)
            read_done[c].record()        # the consumer's reads of the call's set are complete here
            fe.release()
            released[c].record()
    in_flight = sum(not e.query() for e in released)
    # ---- after the window
    torch.cuda.synchronize(cuda)
    print(f"calls in flight when the last of {nchunks} had been enqueued: {in_flight}")
    fe.device_stats()
    assert fe.refused_writes == 0
    log.replay(led)
    og.drain_host(fe, led, "drain")
    fe.finish()
    og.drain_host(fe, led, "end of stream")
    led.finish("unsynchronised window")
    og.check_oracle(led, oracle, nchunks, period, bitrate)          # (asserts that all four block types ran)
    fe.close()
    enc.close()
    return in_flight, read_done, produced


def test_plain(oracle, cuda, monkeypatch):
    """no delay: at this size the device may keep up with Python, so the depth is printed and not asserted"""
    run_window(cuda, monkeypatch, oracle, 32, 12000, [2] * 32)


@pytest.mark.parametrize("point", ["dev_big_back", "dev_small_back", "dev_out", "dev_big_transforms"])
def test_held_up(oracle, cuda, monkeypatch, delay, point):  # noqa: F811
    delay(point)
    depth, _, _ = run_window(cuda, monkeypatch, oracle, 24, 12000, [2] * 24)
    assert depth >= RING + 1, f"{depth} calls in flight: the case does not reach past the ring"


def test_bench_pattern(oracle, cuda, monkeypatch, delay):  # noqa: F811
    """bench.py's round counts: three rings, one per round count, turning at different speeds"""
    delay("dev_big_back")
    depth, _, _ = run_window(cuda, monkeypatch, oracle, 40, 40000, bench_rounds(40))
    assert depth >= RING + 1, f"{depth} calls in flight: the case does not reach past the ring"


def test_managed(oracle, cuda, monkeypatch, delay):  # noqa: F811
    """Managed bitrate, two workspaces: the reservoirs are carried state, and the bitrate manager's choice waits for the
    batches before it.  A managed round runs as plain launches (capi_encoder.cpp, vbm_encoder_device_round_run), whose
    back half passes job_back and not dev_big_back: both points are set, so the back halves are held up either way."""
    delay("dev_big_back", "job_back")
    depth, _, _ = run_window(cuda, monkeypatch, oracle, 20, 6000, [2] * 20, bitrate=og.MANAGED, workspaces="2")
    assert depth >= RING + 1, f"{depth} calls in flight: the case does not reach past the ring"


def test_compact_consumer(oracle, cuda, monkeypatch, delay):  # noqa: F811
    """the consumer copies out with vbm_packets_compact, as a host consumer and the drop-in shim do"""
    delay("dev_out")
    depth, _, _ = run_window(cuda, monkeypatch, oracle, 24, 12000, [2] * 24, compact=True)
    assert depth >= RING + 1, f"{depth} calls in flight: the case does not reach past the ring"


def test_slow_consumer(oracle, cuda, monkeypatch):
    """The consumer's stream is busy for CONSUMER_BUSY_MS before every copy-out and the producer is not held up: left
    alone the producer would be more than three calls ahead, writing the set the consumer is about to read.  The guard
    makes it wait: packets equal the twins and the oracle, and no copy-out of call c ended later than the feeding
    stream got past call c + 3, the call that is handed the same set (one round count: one ring).  The consumer's timed
    event sits between its copies and release(): the guard waits for release()'s event, which comes after it on the same
    stream, so with the guard the time is never negative, by ordering and not by luck.  (The event behind release() is the
    one the depth is counted from.)  With the wait taken out of encode_rounds_device this case fails in the ledger
    ("write 10: identical input, different packets: 693 of 1438 rows differ ... lengths 130 / 173")."""
    n = 24
    depth, read_done, produced = run_window(cuda, monkeypatch, oracle, n, 12000, [2] * n, consumer_busy=True)
    assert depth >= RING + 1, f"{depth} calls in flight: the consumer did not fall behind the ring"
    late = [(c, read_done[c].elapsed_time(produced[c + RING])) for c in range(n - RING)]
    print("ms from the end of copy-out c to the producer passing call c + 3:", [f"{ms:.3f}" for _, ms in late])
    assert all(ms >= 0 for _, ms in late), f"the producer passed call c + 3 before copy-out c had ended: {[(c, ms) for c, ms in late if ms < 0]}"
