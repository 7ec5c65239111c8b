"""PCM intake cases (numpy only): write schedules, their signals, and the oracle driven through a schedule.

How the PCM arrives changes the reference's output: _preextrapolate_helper (lib/block.c:438-484) fits its LPC to
whatever the buffer holds at the vorbis_analysis_wrote that first takes a stream past one long block
(lib/block.c:547-550), and vorbis_analysis_wrote(v, 0) fits the end-of-stream LPC to what is buffered then
(:516-537).  A *schedule* states the delivery exactly; tests/test_intake_cases_cpu.py checks on the oracle alone that
the schedules below make a difference, tests/test_intake_gpu.py and tests/test_compat_intake_gpu.py replay them on
the device.

A schedule is a list of steps:
    ("write", {stream: nsamples})   the next nsamples of each listed stream's signal, one write per stream
    ("drain",)                      every stream hands out blocks until it has none
    ("finish", [streams])           vorbis_analysis_wrote(v, 0)
    ("restart", [streams])          a new logical stream starts in each listed slot (the next signal of the slot)
"""
import ctypes as C

import numpy as np

from tests import orc
from tests.encode_oracle import RECORD_KEEP, record
from tests.signals import burst_signal

# (channels, rate, quality): 256/2048, 512/1024, one size (512), 512/4096, coupled 5.1 256/2048
CLASSES = [(2, 44100, 0.5), (2, 22050, 0.5), (1, 8000, 0.5), (2, 44100, -0.1), (6, 48000, 0.8)]

WRITE_SIZES = [63, 64, 65, 441, 1000, 1023, 1025, 2048, 2049, 4097]
MIXED = [7, 1500, 64, 3, 2049, 333]
# The front end buffers 13 long blocks per stream (vbm_frontend_capacity), centerW = half a long block of them taken
# from the start (lib/block.c:330), so a write of the capacity itself can never fit and is refused; the largest first
# write that is taken is half a long block less.
CAPACITY_BLOCKS = 13
# one schedule per name; "largest": one write of largest_write(), then 1024 at a time
SCHEDULE_NAMES = [str(n) for n in WRITE_SIZES] + ["largest", "mixed"]
WRITE_SAMPLES = 30000


def blocksizes(setup):
    """(short, long) of an orc.Setup"""
    lib = setup.o.lib
    lib.orc_setup_table.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_long), C.c_char_p]
    data, count, kind = C.c_void_p(), C.c_long(), C.create_string_buffer(1)
    rc = lib.orc_setup_table(setup.h, b"info", C.byref(data), C.byref(count), kind)
    assert rc == 0 and count.value >= 4
    info = C.cast(data, C.POINTER(C.c_int))
    return int(info[2]), int(info[3])


def largest_write(bs1):
    return CAPACITY_BLOCKS * bs1 - bs1 // 2


def size_list(name, bs1, total):
    """the write sizes of schedule `name` for a stream of `total` samples (the last one ragged)"""
    if name == "mixed":
        pattern = MIXED
    elif name == "largest":
        pattern = None
    else:
        pattern = [int(name)]
    out, at, k = [], 0, 0
    while at < total:
        n = (largest_write(bs1) if k == 0 else 1024) if pattern is None else pattern[k % len(pattern)]
        n = min(n, total - at)
        out.append(n)
        at += n
        k += 1
    return out


def write_samples(name, bs1):
    """stream length of the write-size schedules (the largest write needs a longer one with 4096-sample blocks)"""
    return max(WRITE_SAMPLES, largest_write(bs1) + 4 * 1024 + 77) if name == "largest" else WRITE_SAMPLES


def write_size_schedule(name, bs1, streams, total, drain_every=1):
    """every stream writes the same sizes; a drain after every drain_every-th write, one before the end, one after"""
    sched = []
    sizes = size_list(name, bs1, total)
    for k, n in enumerate(sizes):
        sched.append(("write", {s: n for s in streams}))
        if (k + 1) % drain_every == 0 or k + 1 == len(sizes):
            sched.append(("drain",))
    sched += [("finish", list(streams)), ("drain",)]
    return sched


def crossing_total(sizes, bs1):
    """samples written when vorbis_analysis_wrote first sees more than one long block (lib/block.c:548)"""
    total = 0
    for n in sizes:
        total += n
        if total > bs1:
            return total
    return None


# Stream 0: only the first packet depends on the write size (tests/test_intake_cases_cpu.py holds the recipe to that).
# Stream 1: for stereo q5 later packets depend on it too — with 2048 samples and more per write the envelope marks
# reach further ahead when a short block is classed impulse or padding (_ve_envelope_mark, lib/envelope.c:683-707).
WRITE_SEEDS = [(816, 1.0), (821, 0.3)]


def write_signals(ch, rate, total, nstreams=2):
    return [burst_signal(ch, rate, total, seed=WRITE_SEEDS[s][0], level=WRITE_SEEDS[s][1]) for s in range(nstreams)]


def onset_signal(ch, rate, N=16384, onset=8000, amp=0.6, seed=1):
    """a tone with a little noise and one 200-sample noise burst of level `amp` at `onset`"""
    rng = np.random.default_rng(seed)
    t = np.arange(N, dtype=np.float64) / rate
    x = np.empty((ch, N), np.float64)
    for c in range(ch):
        x[c] = 0.3 * np.sin(2 * np.pi * 440 * t + c) + 0.01 * rng.uniform(-1, 1, N)
    x[:, onset:onset + 200] += amp * rng.standard_normal((ch, 200))
    return x.astype(np.float32)


ONSET_OFFSETS = [8000 + k for k in range(128)]
ONSET_AMPS = [float(a) for a in np.geomspace(1e-3, 0.6, 32)]


def lockstep_schedule(lengths, chunk=1024):
    """all streams in lock step, `chunk` samples per write and a drain after each (streams of different length stop
    writing when their samples are gone), then the end for all of them"""
    sched = []
    for at in range(0, max(lengths), chunk):
        sched.append(("write", {s: min(chunk, L - at) for s, L in enumerate(lengths) if L > at}))
        sched.append(("drain",))
    sched += [("finish", list(range(len(lengths)))), ("drain",)]
    return sched


def edge_lengths(bs1):
    return [0, 1, 31, 32, 33, 64, 65, 100, bs1 - 1, bs1, bs1 + 1, bs1 + bs1 // 2 - 1, bs1 + bs1 // 2 + 1,
            2 * bs1 - 1, 2 * bs1 + 1, 3 * bs1 + 1]


def edge_length_schedule(lengths, drain_as_you_go, chunk=1024):
    """stream s holds lengths[s] samples, written `chunk` at a time; its end is declared in the step after its last
    write.  drain_as_you_go: a drain after every write and before every end; otherwise none until all have ended."""
    sched = []
    nsteps = max((L + chunk - 1) // chunk for L in lengths)
    for k in range(nsteps + 1):
        writes = {s: min(chunk, L - k * chunk) for s, L in enumerate(lengths) if L > k * chunk}
        ending = [s for s, L in enumerate(lengths) if (L + chunk - 1) // chunk == k]
        if ending:
            sched.append(("finish", ending))
        if writes:
            sched.append(("write", writes))
        if drain_as_you_go:
            sched.append(("drain",))
    if not drain_as_you_go:
        sched.append(("drain",))
    return sched


def edge_signals(ch, rate, lengths):
    """one signal per length: loud from its first sample on (the pre-extrapolation has something to fit)"""
    out = []
    for s, L in enumerate(lengths):
        rng = np.random.default_rng(300 + s)
        t = np.arange(L, dtype=np.float64) / rate
        x = np.stack([0.4 * np.cos(2 * np.pi * 523.0 * t + c) + 0.05 * rng.uniform(-1, 1, L) for c in range(ch)])
        out.append(x.astype(np.float32).reshape(ch, L))
    return out


def _blocks(st, seq):
    """hand out every ready block of orc.Stream st as its record (tests/encode_oracle.py), reading the block's own
    fields and the packet alone: these schedules have thousands of drains"""
    lib = st.lib
    info, i64, nb = (C.c_int * 8)(), (C.c_int64 * 2)(), C.c_long()
    while lib.orc_analysis_blockout(st.v, st.vb) == 1:
        lib.orc_analysis(st.v, st.vb)
        lib.orc_block_info(st.vb, info)
        lib.orc_block_info64(st.vb, i64)
        pk = lib.orc_block_packet(st.vb, C.byref(nb))
        seq.append(record(dict(zip(RECORD_KEEP, (info[0], info[1], info[2], info[5], info[6], i64[0], i64[1],
                                                 C.string_at(pk, nb.value))))))


def oracle_run(oracle, setup, signals, schedule):
    """Replays `schedule` on one orc.Stream per logical stream.  signals[s]: the (ch, N) signal of slot s, or a list of
    them, one per logical stream that lives in the slot (("restart", ...) moves on to the next).  Returns
    want[s] = [sequence of the slot's first logical stream, of its second, ...]."""
    slots = sorted({s for step in schedule if step[0] != "drain" for s in step[1]})
    sigs = {s: (signals[s] if isinstance(signals[s], (list, tuple)) else [signals[s]]) for s in slots}
    live, at, gen = {}, {}, {s: 0 for s in slots}
    want = {s: [[]] for s in slots}

    def stream(s):
        if s not in live:
            live[s] = orc.Stream(setup)
            oracle.lib.orc_stream_set_capture(live[s].v, 0)
            at[s] = 0
        return live[s]

    for step in schedule:
        if step[0] == "write":
            for s, n in step[1].items():
                st = stream(s)
                sig = sigs[s][gen[s]]
                assert n > 0 and at[s] + n <= sig.shape[1], (s, at[s], n)
                st.write(sig[:, at[s]:at[s] + n])
                at[s] += n
        elif step[0] == "drain":
            for s, st in live.items():
                _blocks(st, want[s][-1])
        elif step[0] == "finish":
            for s in step[1]:
                stream(s).finish()
        elif step[0] == "restart":
            for s in step[1]:
                if s in live:
                    live.pop(s).close()
                gen[s] += 1
                want[s].append([])
        else:
            raise ValueError(step[0])
    for st in live.values():
        st.close()
    return want
