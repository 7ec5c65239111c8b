"""PCM intake of the device front end at every write size, stream length and burst onset (tests/intake_cases.py)
against the oracle driven through the identical writes, drains and ends.  Per stream, in order:
(lW, W, nW, block type, e_o_s, granulepos, packetno) and the packet bytes are the oracle's.  No tolerance.

What the delivery changes in the reference, and so here: the start-of-stream LPC is fitted at the write that first
takes a stream past one long block (lib/block.c:547-550), the end-of-stream LPC to what is buffered at the end
(:516-537), and a short block's type to the envelope marks known when it is carved (lib/envelope.c:683-707)."""
import numpy as np
import pytest
import torch

from tests import intake_cases as ic
from tests import orc
from tests.test_frontend_gpu import collect_device, drain

pytestmark = pytest.mark.gpu

IDS = {cls: f"{cls[0]}ch-{cls[1]}-q{cls[2]:g}" for cls in ic.CLASSES}
STEREO_Q5, STEREO_22, MONO_8, STEREO_QNEG, SURROUND = ic.CLASSES


def class_id(cls):
    return IDS[cls]


_osetups, _wanted = {}, {}


def osetup(oracle, cls):
    if cls not in _osetups:
        _osetups[cls] = orc.Setup(oracle, *cls)
    return _osetups[cls]


def wanted(oracle, cls, key, signals, schedule):
    """the oracle's sequences for a (class, case): computed once, shared by the tests that replay the case"""
    if (cls, key) not in _wanted:
        _wanted[(cls, key)] = ic.oracle_run(oracle, osetup(oracle, cls), signals, schedule)
    return _wanted[(cls, key)]


class DeviceRun:
    """One FrontEnd driven through a schedule.  how: "write" (FrontEnd.write: every stream, one size), "streams"
    (write_streams, one call per distinct size of a step) or "strided" (write_streams_strided from a device arena:
    by slot, channel stride larger than any write, base one float off 16-byte alignment).
    rounds: None = host-built rounds until nothing is left; n = every drain runs n device-built rounds first, and where
    an end, a restart or nothing follows, host-built rounds then carve what is left (the end-of-stream fit wants the
    buffer drained).  device_count[s] / device_eos[s]: blocks / e_o_s blocks of slot s that device-built rounds carved."""
    ARENA = 4100

    def __init__(self, cuda, cls, nstreams, how, rounds=None):
        import vorbis_aotuv_lancer_amd as v
        self.v, self.cuda, self.how, self.rounds = v, cuda, how, rounds
        self.setup = v.Setup(*cls)
        self.S, self.ch = nstreams, cls[0]
        lanes = v.lib.vbm_device_round_lanes(self.setup._h, nstreams) if rounds else None
        self.enc = v.Encoder(self.setup, nstreams, max_batch=lanes)
        self.fe = v.FrontEnd(self.enc)
        self.got = [[] for _ in range(nstreams)]
        self.done = {s: [] for s in range(nstreams)}     # finished logical streams of a slot
        self.at = [0] * nstreams
        self.gen = [0] * nstreams
        self.device_blocks = 0
        self.device_count = [0] * nstreams
        self.device_eos = [0] * nstreams
        if how == "strided":
            self.flat = torch.zeros(1 + nstreams * self.ch * self.ARENA, dtype=torch.float32, device=cuda)
            self.arena = self.flat[1:].view(nstreams, self.ch, self.ARENA)
            assert self.arena.data_ptr() % 16 == 4

    def signal(self, signals, s):
        sig = signals[s]
        return sig[self.gen[s]] if isinstance(sig, (list, tuple)) else sig

    def write(self, signals, sizes):
        pcs = {}
        for s, n in sizes.items():
            sig = self.signal(signals, s)
            assert n > 0 and self.at[s] + n <= sig.shape[1]
            pcs[s] = sig[:, self.at[s]:self.at[s] + n]
            self.at[s] += n
        if self.how == "write":
            n = next(iter(sizes.values()))
            assert sorted(sizes) == list(range(self.S)) and all(m == n for m in sizes.values())
            self.fe.write(torch.from_numpy(np.stack([pcs[s] for s in range(self.S)])).to(self.cuda).contiguous())
            return
        for n in sorted(set(sizes.values())):
            ids = [s for s in sorted(sizes) if sizes[s] == n]
            if self.how == "streams":
                self.fe.write_streams(ids, torch.from_numpy(np.stack([pcs[s] for s in ids])).to(self.cuda).contiguous())
            else:
                assert n < self.ARENA
                for s in ids:
                    self.arena[s, :, :n] = torch.from_numpy(np.ascontiguousarray(pcs[s])).to(self.cuda)
                torch.cuda.synchronize()
                self.fe.write_streams_strided(ids, self.arena, n, self.ch * self.ARENA, self.ARENA, by_slot=True)

    def run(self, signals, schedule):
        for k, step in enumerate(schedule):
            if step[0] == "write":
                self.write(signals, step[1])
            elif step[0] == "drain":
                ahead = schedule[k + 1][0] if k + 1 < len(schedule) else "finish"
                if self.rounds:
                    before = [len(g) for g in self.got]
                    out = self.fe.encode_rounds_device(nrounds=self.rounds)
                    self.device_blocks += collect_device(self.got, self.fe, out)
                    for s in range(self.S):
                        self.device_count[s] += len(self.got[s]) - before[s]
                        self.device_eos[s] += sum(m[4] for m, _ in self.got[s][before[s]:])
                if not self.rounds or ahead != "write":
                    drain(self.fe, self.got)
            elif step[0] == "finish":
                self.fe.finish(step[1])
            elif step[0] == "restart":
                for s in step[1]:
                    self.done[s].append(self.got[s])
                    self.got[s] = []
                    self.at[s] = 0
                    self.gen[s] += 1
                self.fe.restart_streams(step[1])
        if self.rounds:
            self.fe.device_stats()
            assert self.fe.refused_writes == 0
        return {s: self.done[s] + [self.got[s]] for s in range(self.S)}

    def close(self):
        self.fe.close()
        self.enc.close()


def compare(got, want, label=""):
    for s in sorted(want):
        assert len(got[s]) == len(want[s]), (label, s)
        for g, (a, b) in enumerate(zip(got[s], want[s])):
            assert [m for m, _ in a] == [m for m, _ in b], f"{label} stream {s}.{g}: block sequence differs from the oracle"
            bad = [i for i in range(len(b)) if a[i][1] != b[i][1]]
            assert not bad, f"{label} stream {s}.{g}: packet {bad[0]} of {len(b)} differs from the oracle"


def block_types(want):
    return {m[3] for seqs in want.values() for seq in seqs for m, _ in seq}


def need_types(cls, want):
    # two block sizes: long and short blocks both occur; one size: types 0 and 1
    types = block_types(want)
    if cls == MONO_8:
        assert types >= {0, 1}, types
    else:
        assert types & {0, 1} and 3 in types, types


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
    compare(run.run(signals, schedule), want, name)
    run.close()


@pytest.mark.parametrize("cls", [c for c in ic.CLASSES if c != STEREO_QNEG], ids=class_id)
def test_one_sample_writes(oracle, cuda, cls):
    """a long block and 300 samples, one sample per write, a drain every 64th: the start is extrapolated at the write
    that makes it one long block and one sample (every class whose long block is at most 2048 samples)"""
    bs1 = ic.blocksizes(osetup(oracle, cls))[1]
    assert bs1 <= 2048
    signals, schedule, want = write_case(oracle, cls, "1", drain_every=64, total=bs1 + 300)
    run = DeviceRun(cuda, cls, 2, "write")
    compare(run.run(signals, schedule), want)
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
    compare(run.run(signals, schedule), want, how)
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
    compare(run.run(signals, schedule), want)
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
    compare(got, want)
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
    compare(run.run(signals, schedule), want, name)
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
    compare(run.run(signals, schedule[cut:]), want)
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
    compare(run.run(signals, schedule), want)
    run.close()


@pytest.mark.parametrize("cls", [STEREO_Q5, STEREO_22], ids=class_id)
def test_onset_amplitudes(oracle, cuda, cls):
    """the burst from far below the detector's trigger level to far above it, 32 levels"""
    signals = [ic.onset_signal(cls[0], cls[1], amp=amp) for amp in ic.ONSET_AMPS]
    schedule, want = onset_case(oracle, cls, "amplitudes", signals)
    assert len({short_blocks(want[s][0]) for s in want}) >= 2
    run = DeviceRun(cuda, cls, len(signals), "write")
    compare(run.run(signals, schedule), want)
    run.close()
