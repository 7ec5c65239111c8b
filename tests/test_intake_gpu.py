"""PCM intake of the device front end at every write size, stream length and burst onset (tests/intake_cases.py)
against the oracle driven through the identical writes, drains and ends.  Per stream, in order:
(lW, W, nW, block type, e_o_s, granulepos, packetno) and the packet bytes are the oracle's.  No tolerance.

What the delivery changes in the reference, and so here: the start-of-stream LPC is fitted at the write that first
takes a stream past one long block (lib/block.c:547-550), the end-of-stream LPC to what is buffered at the end
(:516-537), and a short block's type to the envelope marks known when it is carved (lib/envelope.c:683-707)."""
import pytest
import torch

from tests import intake_cases as ic
from tests.encode_calls import DeviceRun, compare_slots, need_types, osetup, wanted

pytestmark = pytest.mark.gpu

IDS = {cls: f"{cls[0]}ch-{cls[1]}-q{cls[2]:g}" for cls in ic.CLASSES}
STEREO_Q5, STEREO_22, MONO_8, STEREO_QNEG, SURROUND = ic.CLASSES


def class_id(cls):
    return IDS[cls]


# ---- a. write sizes through FrontEnd.write -------------------------------------------------------------------------
def write_case(oracle, cls, name, drain_every=1, total=None):
    bs1 = ic.blocksizes(osetup(oracle, cls))[1]
    total = total or ic.write_samples(name, bs1)
    signals = ic.write_signals(cls[0], cls[1], total)
    schedule = ic.write_size_schedule(name, bs1, [0, 1], total, drain_every)
    return signals, schedule, wanted(oracle, cls, ("write", name, total, drain_every), signals, schedule)


@pytest.mark.parametrize("name", ic.SCHEDULE_NAMES)
@pytest.mark.parametrize("cls", ic.CLASSES, ids=class_id)
def test_write_sizes(oracle, cuda, cls, name):
    """"largest": the biggest first write the front end takes (its capacity less the half long block every buffer
    starts with); the capacity itself is refused, as it always was (test_api_edges_gpu.py: can never fit)"""
    signals, schedule, want = write_case(oracle, cls, name)
    need_types(cls, want)
    run = DeviceRun(cuda, cls, 2, "write")
    if name == "largest":
        bs1 = run.setup.blocksizes[1]
        assert run.fe.capacity - bs1 // 2 == ic.largest_write(bs1)
        with pytest.raises(run.v.VbmError):
            run.fe.write(torch.zeros((2, cls[0], run.fe.capacity), device=cuda))
        assert run.fe.max_buffered == bs1 // 2                       # nothing was taken
    compare_slots(run.run(signals, schedule), want, name)
    run.close()


@pytest.mark.parametrize("cls", [c for c in ic.CLASSES if c != STEREO_QNEG], ids=class_id)
def test_one_sample_writes(oracle, cuda, cls):
    """a long block and 300 samples, one sample per write, a drain every 64th: the start is extrapolated at the write
    that makes it one long block and one sample (every class whose long block is at most 2048 samples)"""
    bs1 = ic.blocksizes(osetup(oracle, cls))[1]
    assert bs1 <= 2048
    signals, schedule, want = write_case(oracle, cls, "1", drain_every=64, total=bs1 + 300)
    run = DeviceRun(cuda, cls, 2, "write")
    compare_slots(run.run(signals, schedule), want)
    run.close()


# ---- b. different sizes in one step --------------------------------------------------------------------------------
PER_STREAM = [63, 64, 65, 441, 1000, 1023, 1024, 1025, 2048, 2049, 4097, "mixed"]


def mixed_step_case(oracle, cls):
    bs1 = ic.blocksizes(osetup(oracle, cls))[1]
    total = ic.WRITE_SAMPLES
    sizes = [ic.size_list(str(n), bs1, total) for n in PER_STREAM]
    signals = [ic.burst_signal(cls[0], cls[1], total, seed=840 + s, level=1.0 if s % 3 else 0.2) for s in range(len(sizes))]
    schedule, ended = [], set()
    for k in range(max(len(z) for z in sizes) + 1):
        ending = [s for s, z in enumerate(sizes) if len(z) == k]
        if ending:                                                   # (the step before ended with a drain)
            schedule.append(("finish", ending))
        writes = {s: z[k] for s, z in enumerate(sizes) if k < len(z)}
        if writes:
            schedule.append(("write", writes))
        schedule.append(("drain",))
    return signals, schedule, wanted(oracle, cls, "mixed step", signals, schedule)


@pytest.mark.parametrize("how", ["streams", "strided"])
@pytest.mark.parametrize("cls", [STEREO_Q5, SURROUND], ids=class_id)
def test_different_sizes_in_one_step(oracle, cuda, cls, how):
    """twelve streams, each with its own write size, one call per distinct size and step: after an odd write every
    later one lands off 16-byte alignment in the buffer, so the 1500- and 64-sample writes of the mixed stream and the
    1000-sample writes from the unaligned arena take the append kernels' scalar path with vals % 4 == 0"""
    signals, schedule, want = mixed_step_case(oracle, cls)
    need_types(cls, want)
    run = DeviceRun(cuda, cls, len(PER_STREAM), how)
    compare_slots(run.run(signals, schedule), want, how)
    run.close()


# ---- c. stream lengths ---------------------------------------------------------------------------------------------
def length_case(oracle, cls, drain_as_you_go):
    bs1 = ic.blocksizes(osetup(oracle, cls))[1]
    lengths = ic.edge_lengths(bs1)
    n = len(lengths)
    second = [ic.burst_signal(cls[0], cls[1], 20000, seed=870 + s) for s in range(n)]
    signals = [[a, b] for a, b in zip(ic.edge_signals(cls[0], cls[1], lengths), second)]
    schedule = ic.edge_length_schedule(lengths, drain_as_you_go)
    schedule.append(("restart", list(range(n))))                    # every slot takes a new stream
    schedule += ic.lockstep_schedule([20000] * n)
    return lengths, signals, schedule, wanted(oracle, cls, ("lengths", drain_as_you_go), signals, schedule)


@pytest.mark.parametrize("drain_as_you_go", [True, False], ids=["drained", "undrained"])
@pytest.mark.parametrize("cls", [STEREO_Q5, STEREO_22, MONO_8], ids=class_id)
def test_stream_lengths(oracle, cuda, cls, drain_as_you_go):
    """streams that end before (or just after) they ever held one long block: no pre-extrapolation at 32 samples and
    fewer, the LPC on a very short run above that (k_fe_extrapolate mode 1), then the slot's next stream"""
    lengths, signals, schedule, want = length_case(oracle, cls, drain_as_you_go)
    for s in range(len(lengths)):
        assert len(want[s][0]) >= 1 and want[s][0][-1][0][4] == 1
    run = DeviceRun(cuda, cls, len(lengths), "streams")
    compare_slots(run.run(signals, schedule), want)
    run.close()


# ---- d. fill, then drain -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [STEREO_Q5, STEREO_QNEG], ids=class_id)
def test_fill_then_drain(oracle, cuda, cls):
    """1024-sample writes with no round in between until the next one would be refused, then a complete drain — the
    longest run of pending search steps, marks and origin compaction — three times over"""
    run = DeviceRun(cuda, cls, 2, "write")
    fe = run.fe
    per_fill = fe.capacity // 1024 + 1
    total = 3 * per_fill * 1024
    signals = [ic.burst_signal(cls[0], cls[1], total, seed=890 + s, period=5000) for s in range(2)]
    schedule, fills = [], []
    for _ in range(3):
        n = 0
        while fe.max_buffered + 1024 <= fe.capacity:
            step = ("write", {0: 1024, 1: 1024})
            run.run(signals, [step])
            schedule.append(step)
            n += 1
        fills.append(n)
        with pytest.raises(run.v.VbmError):                          # the next write is refused, and takes nothing
            fe.write(torch.zeros((2, cls[0], 1024), device=cuda))
        run.run(signals, [("drain",)])
        schedule.append(("drain",))
    assert min(fills) >= (fe.capacity - 2 * run.setup.blocksizes[1]) // 1024, fills
    tail = [("finish", [0, 1]), ("drain",)]
    got = run.run(signals, tail)
    want = ic.oracle_run(oracle, osetup(oracle, cls), signals, schedule + tail)
    need_types(cls, want)
    compare_slots(got, want)
    run.close()


# ---- e. rounds built on the device ---------------------------------------------------------------------------------
def device_rounds_per_write(setup, vals):
    # a round moves a stream by half a long block at the most: enough rounds to keep up with long blocks and two to
    # spare for runs of short ones (what those leave behind waits in the buffer: 13 long blocks hold 30000 samples)
    return max(2, 2 * vals // setup.blocksizes[1] + 2)


@pytest.mark.parametrize("name", ["441", "1025", "4097", "mixed"])
def test_write_sizes_with_device_built_rounds(oracle, cuda, monkeypatch, name):
    monkeypatch.setenv("VBM_WORKSPACES", "4")
    cls = STEREO_Q5
    signals, schedule, want = write_case(oracle, cls, name)
    vals = max(ic.MIXED) if name == "mixed" else int(name)
    run = DeviceRun(cuda, cls, 2, "write", rounds=1)
    run.rounds = device_rounds_per_write(run.setup, vals)
    compare_slots(run.run(signals, schedule), want, name)
    assert run.device_blocks > len(want[0][0])                      # most blocks came out of device-built rounds
    run.close()


def test_stream_lengths_with_device_built_rounds(oracle, cuda, monkeypatch):
    """drained order only: without drains there is no round for the device to build.  Two device-built rounds at every
    drain, so a stream that has just ended (pre-extrapolated at its end, if it never held a long block) has its first
    two blocks carved by device-built rounds — for the streams of 100 samples and fewer that is all of them, the e_o_s
    block included."""
    monkeypatch.setenv("VBM_WORKSPACES", "4")
    cls = STEREO_Q5
    lengths, signals, schedule, want = length_case(oracle, cls, True)
    cut = next(k for k, step in enumerate(schedule) if step[0] == "restart")
    run = DeviceRun(cuda, cls, len(lengths), "streams", rounds=2)
    run.run(signals, schedule[:cut])
    for s, L in enumerate(lengths):                                  # the short streams, before any slot is reused
        assert run.device_count[s] >= min(2, len(want[s][0])), (L, run.device_count[s])
        if L <= 100:
            assert len(want[s][0]) <= 2 and run.device_eos[s] == 1 and run.device_count[s] == len(want[s][0]), L
    assert sum(run.device_eos) >= 8
    compare_slots(run.run(signals, schedule[cut:]), want)
    run.close()


# ---- f. onsets -----------------------------------------------------------------------------------------------------
def onset_case(oracle, cls, key, signals):
    schedule = ic.lockstep_schedule([sig.shape[1] for sig in signals])
    return schedule, wanted(oracle, cls, key, signals, schedule)


def short_blocks(seq):
    return sum(1 for m, _ in seq if m[1] == 0)


def test_onset_offsets(oracle, cuda):
    """the same burst at 128 consecutive offsets (two search steps of the envelope detector)"""
    cls = STEREO_Q5
    signals = [ic.onset_signal(cls[0], cls[1], onset=onset) for onset in ic.ONSET_OFFSETS]
    schedule, want = onset_case(oracle, cls, "offsets", signals)
    assert len({tuple(m[:4] for m, _ in want[s][0]) for s in want}) >= 2
    run = DeviceRun(cuda, cls, len(signals), "write")
    compare_slots(run.run(signals, schedule), want)
    run.close()


@pytest.mark.parametrize("cls", [STEREO_Q5, STEREO_22], ids=class_id)
def test_onset_amplitudes(oracle, cuda, cls):
    """the burst from far below the detector's trigger level to far above it, 32 levels"""
    signals = [ic.onset_signal(cls[0], cls[1], amp=amp) for amp in ic.ONSET_AMPS]
    schedule, want = onset_case(oracle, cls, "amplitudes", signals)
    assert len({short_blocks(want[s][0]) for s in want}) >= 2
    run = DeviceRun(cuda, cls, len(signals), "write")
    compare_slots(run.run(signals, schedule), want)
    run.close()
