"""The long blocks of a device-built call's first round are read where they lie: k_fe_round_commit leaves every lane's
float offset into the front end's channel buffers, the big batch's window + MDCT and window + FFT kernels take their
blocks from there (csrc/mdct_kernel.h: vbm_block_src) and the round's type-3 gather is gone.  Every other job (the small
block types, the long blocks of a call's later rounds, and every job of the plain-launch form) keeps its gathered copy.

A few streams per class, packet for packet and through PacketInfo against the oracle replaying the same writes:

  origins       unequal first writes and block switching at different moments put the streams at different origins
                and parities in the same round; the buffers are the smallest that take four rounds per write without a
                refused write (VBM_FE_BUFFER_BLOCKS=12), so every stream compacts several times
  rounds        four rounds per call, and some writes of three long blocks: the later rounds' long blocks take the
                gathered path in the same call as the direct one
  poison        the front end's staging buffers and round lists are filled with 0xFF before every call (group of calls):
                a transform that still read the type-3 staging region would see NaNs
  held up       the big batch's transforms, the buffer shift and the append of a write, each held up by a spin kernel
                while the later rounds of the call and the next write and call queue behind
  plain form    stage profiling and a managed setup run the rounds as plain launches, which keep the gather; so does a
                setup with 4096-sample long blocks
  empty / full  a first round without a long block (the start of the streams), and first rounds in which every
                stream delivers one (twin streams in lock step): count 0 and count == cap of the type-3 region"""
import numpy as np
import pytest

from tests import intake_cases as ic
from tests.encode_calls import MANAGED, DeviceRun, collect_device, compare_slots, delay, drain, osetup  # noqa: F401 (delay: fixture)
from tests.signals import burst_signal, synth_signal

pytestmark = pytest.mark.gpu

BUFFER_BLOCKS = 12
ROUNDS = 4
STEREO, MONO, SURROUND = (2, 44100, 0.5), (1, 44100, 0.5), (6, 48000, 0.8)
LONG4096 = (2, 44100, -0.1)      # long blocks of 4096 samples: no direct form, the first round's long blocks are gathered
_cases, _want = {}, {}


def mixed_case(cls, S, nwrites=44):
    """S streams of different signals: an unequal first write, then 1024 samples per write, three long blocks for every
    fourth stream twice on the way -> (signals, schedule)"""
    key = (cls[0], cls[1], S, nwrites)
    if key not in _cases:
        sizes = [{s: 640 + 388 * s for s in range(S)}]
        big = 6144 if cls == LONG4096 else 3072           # what three long blocks move a stream on by
        for w in range(nwrites):
            sizes.append({s: big if w in (10, 25) and s % 4 == 1 else 1024 for s in range(S)})
        sched = []
        for sz in sizes:
            sched += [("write", sz), ("drain",)]
        sched += [("finish", list(range(S))), ("drain",)]
        sigs = []
        for s in range(S):
            total = sum(sz[s] for sz in sizes)
            make = burst_signal if s % 2 == 0 else synth_signal
            kw = dict(period=7000) if s % 2 == 0 else {}
            sigs.append(make(cls[0], cls[1], total, seed=900 + s, level=1.0 if s % 3 else 0.05, **kw))
        _cases[key] = (sigs, sched)
    return _cases[key]


def twin_case(cls, S, nwrites=30):
    """S streams of one quiet, steady signal in lock step: whenever it is in long blocks, all of them are"""
    key = ("twins", cls[0], cls[1], S, nwrites)
    if key not in _cases:
        t = np.arange(nwrites * 1024, dtype=np.float64) / cls[1]
        rng = np.random.default_rng(5)
        one = np.stack([0.3 * np.sin(2 * np.pi * 440 * t + c) + 0.01 * rng.uniform(-1, 1, len(t))
                        for c in range(cls[0])]).astype(np.float32)
        _cases[key] = ([one] * S, ic.lockstep_schedule([one.shape[1]] * S))
    return _cases[key]


def want_of(oracle, cls, name, sigs, sched):
    key = (cls, name, len(sigs))
    if key not in _want:
        _want[key] = ic.oracle_run(oracle, osetup(oracle, cls), sigs, sched)
    return _want[key]


def buffers(v, fe, S):
    base, parity, cur = (np.zeros(S, np.int32) for _ in range(3))
    shift = np.zeros(2 + S, np.int32)
    assert v.lib.vbm_debug_frontend_buffers(fe._h, base.ctypes.data, parity.ctypes.data, cur.ctypes.data,
                                            shift.ctypes.data, None, 0) == 0
    return base, parity


def run_case(cuda, monkeypatch, cls, sigs, sched, depth=1, profile=False):
    """The schedule on the device: every drain is ROUNDS device-built rounds (host-built ones where no write follows).
    depth: calls enqueued before the first of them is collected; the front end is poisoned before every such group.
    -> (records by slot, facts about the rounds that ran)"""
    monkeypatch.setenv("VBM_FE_BUFFER_BLOCKS", str(BUFFER_BLOCKS))
    S = len(sigs)
    run = DeviceRun(cuda, cls, S, "streams", rounds=ROUNDS)
    v, fe = run.v, run.fe
    if profile:
        run.enc.profile_begin(16)       # (stage times of the first 16 calls; the plain-launch form until profile_end)
    facts = dict(direct_and_gathered=0, empty_first=0, full_first=0, origins=0, parities=0, flips=np.zeros(S, np.int64))
    parity_was = np.zeros(S, np.int32)
    held = []

    def flush():
        nonlocal parity_was
        for out in held:
            collect_device(run.got, fe, out)
            c = out[3].cpu().numpy()
            facts["direct_and_gathered"] += bool(c[0, 3] > 0 and (c[1:, 3] > 0).any())
            facts["empty_first"] += bool(c[0, 3] == 0)
            facts["full_first"] += bool(c[0, 3] == S)
        held.clear()
        base, parity = buffers(v, fe, S)
        facts["origins"] += len(set(base.tolist())) > 1
        facts["parities"] += len(set(parity.tolist())) > 1
        facts["flips"] += parity != parity_was
        parity_was = parity

    for k, step in enumerate(sched):
        ahead = sched[k + 1][0] if k + 1 < len(sched) else "finish"
        if step[0] == "write":
            sizes = step[1]
            # every stream, one size: the append that waits for nothing on the host (a later write queues behind)
            run.how = "write" if sorted(sizes) == list(range(S)) and len(set(sizes.values())) == 1 else "streams"
            run.write(sigs, sizes)
        elif step[0] == "drain":
            if not held:
                fe.join()
                fe.debug_poison(0xFF)
            held.append(fe.encode_rounds_device(nrounds=ROUNDS))
            if len(held) >= depth or ahead != "write":
                flush()
            if ahead != "write":
                drain(fe, run.got)
        else:
            assert step[0] == "finish" and not held
            fe.finish(step[1])
    fe.device_stats()
    assert fe.refused_writes == 0
    if profile:
        run.enc.profile_end()
    got = {s: [run.got[s]] for s in range(S)}
    run.close()
    return got, facts


def check_mixed(facts, label):
    assert facts["direct_and_gathered"] > 0, (label, "no call with long blocks in its first and in a later round")
    assert facts["empty_first"] > 0, (label, "no first round without a long block")
    assert facts["origins"] > 0 and facts["parities"] > 0, (label, facts)
    assert facts["flips"].min() >= 3, (label, "compactions per stream", facts["flips"])


@pytest.mark.parametrize("cls,S,nwrites", [(STEREO, 10, 44), (MONO, 7, 44), (SURROUND, 6, 44), (LONG4096, 5, 80)],
                         ids=["2ch", "1ch", "6ch", "2ch_4096"])
def test_direct_blocks_against_the_oracle(oracle, cuda, monkeypatch, cls, S, nwrites):
    sigs, sched = mixed_case(cls, S, nwrites)
    got, facts = run_case(cuda, monkeypatch, cls, sigs, sched)
    compare_slots(got, want_of(oracle, cls, "mixed", sigs, sched), f"{cls}")
    check_mixed(facts, cls)


def test_full_and_empty_type3_region(oracle, cuda, monkeypatch):
    sigs, sched = twin_case(STEREO, 6)
    got, facts = run_case(cuda, monkeypatch, STEREO, sigs, sched)
    compare_slots(got, want_of(oracle, STEREO, "twins", sigs, sched), "twins")
    assert facts["full_first"] > 0 and facts["empty_first"] > 0, facts


@pytest.mark.parametrize("point", ["dev_big_transforms", "fe_shift", "fe_write"])
def test_held_up(oracle, cuda, monkeypatch, delay, point):
    sigs, sched = mixed_case(STEREO, 10)
    delay(point)
    got, facts = run_case(cuda, monkeypatch, STEREO, sigs, sched, depth=2)
    compare_slots(got, want_of(oracle, STEREO, "mixed", sigs, sched), point)
    check_mixed(facts, point)


def test_plain_launches_profiled(oracle, cuda, monkeypatch):
    """stage profiling: plain launches, the big batch's transforms on a stream beside the shift: it keeps its gather"""
    sigs, sched = mixed_case(STEREO, 10)
    got, facts = run_case(cuda, monkeypatch, STEREO, sigs, sched, profile=True)
    compare_slots(got, want_of(oracle, STEREO, "mixed", sigs, sched), "profiled")
    check_mixed(facts, "profiled")


def test_plain_launches_managed(oracle, cuda, monkeypatch):
    cls = (2, 44100, None, MANAGED)
    sigs, sched = mixed_case(cls, 10)
    got, facts = run_case(cuda, monkeypatch, cls, sigs, sched)
    compare_slots(got, want_of(oracle, cls, "mixed", sigs, sched), "managed")
    check_mixed(facts, "managed")
