"""FrontEnd.write_ragged (vbm_frontend_write_ragged): every listed stream with a size of its own in ONE call, taken
straight from a store of whole signals, against the oracle driven through the identical schedule — byte for byte —
and against the grouped path (write_streams once per distinct size of a step)."""
import numpy as np
import pytest
import torch

from tests import intake_cases as ic
from tests.encode_calls import DeviceRun, compare_slots, need_types, osetup, wanted
from tests.signals import burst_signal

pytestmark = pytest.mark.gpu

STEREO_Q5, MONO_8, SURROUND = (2, 44100, 0.5), (1, 8000, 0.5), (6, 48000, 0.8)
IDS = {STEREO_Q5: "2ch-44100-q0.5", MONO_8: "1ch-8000-q0.5", SURROUND: "6ch-48000-q0.8"}

# the write sizes of the intake suite, in an order that starts stream 0 with three sizes that keep it on 16-byte
# boundaries (its part of the store is aligned too): stream s writes ORDER[(step + s) % 10], so the sizes of a step
# all differ and every stream meets every size
ORDER = [64, 2048, 1000, 63, 65, 441, 1023, 1025, 2049, 4097]
NS, STEPS = 5, 14
SOLO_STEP, SOLO_STREAM = 4, 2        # a step that lists one stream (from a staged [ch][vals] tensor: ch_strides=None)
EARLY_END = 8                        # the last stream ends after this step, its neighbours go on


def mixed_schedule():
    assert sorted(ORDER) == sorted(ic.WRITE_SIZES)
    sched = []
    for k in range(STEPS):
        if k == EARLY_END + 1:
            sched.append(("finish", [NS - 1]))
        if k == SOLO_STEP:
            writes = {SOLO_STREAM: ORDER[(k + SOLO_STREAM) % 10]}
        else:
            writes = {s: ORDER[(k + s) % 10] for s in range(NS) if s < NS - 1 or k <= EARLY_END}
            assert len(set(writes.values())) == len(writes)
        sched += [("write", writes), ("drain",)]
    sched += [("finish", list(range(NS - 1))), ("drain",)]
    return sched


def totals(schedule):
    t = [0] * NS
    for step in schedule:
        if step[0] == "write":
            for s, n in step[1].items():
                t[s] += n
    return t


def mixed_case(oracle, cls):
    schedule = mixed_schedule()
    signals = [burst_signal(cls[0], cls[1], n, seed=950 + s, period=4000, level=1.0 if s % 2 else 0.3)
               for s, n in enumerate(totals(schedule))]
    return signals, schedule, wanted(oracle, cls, "ragged mixed", signals, schedule)


class RaggedRun(DeviceRun):
    """DeviceRun whose writes go through write_ragged, one call per step, ids in descending order.  Store: stream s's
    channel c at base[s] + c * stride[s]; even streams start on a 16-byte boundary with a stride that keeps every
    channel there, odd streams start one float off with an odd stride; every stride is larger than any write."""

    def __init__(self, cuda, cls, signals):
        super().__init__(cuda, cls, len(signals), "streams")
        self.base, self.stride, total = [], [], 0
        for s, sig in enumerate(signals):
            n = sig.shape[1]
            total = (total + 3) & ~3
            if s % 2:
                total += 1
            self.base.append(total)
            self.stride.append(((n + 3) & ~3) + 8 if s % 2 == 0 else (n | 1) + 2)
            total += self.ch * self.stride[s]
        host = np.zeros(total, np.float32)
        for s, sig in enumerate(signals):
            host[self.base[s]:self.base[s] + self.ch * self.stride[s]].reshape(self.ch, -1)[:, :sig.shape[1]] = sig
        self.store = torch.from_numpy(host).to(cuda)
        assert self.store.data_ptr() % 16 == 0
        self.wide = self.narrow = 0            # writes whose source allows 16 bytes per lane / does not

    def write(self, signals, sizes):
        slots = sorted(sizes, reverse=True)
        vals = [sizes[s] for s in slots]
        if len(slots) == 1:
            s = slots[0]
            staged = torch.from_numpy(np.ascontiguousarray(signals[s][:, self.at[s]:self.at[s] + vals[0]])).to(self.cuda)
            self.fe.write_ragged(slots, staged, [0], vals)
        else:
            offsets = [self.base[s] + self.at[s] for s in slots]
            for s, off, n in zip(slots, offsets, vals):
                # (a stream's buffer fill stays a multiple of 4 while all its writes are: blocks move it by multiples of 4)
                ok = off % 4 == 0 and n % 4 == 0 and self.at[s] % 4 == 0 and (self.ch == 1 or self.stride[s] % 4 == 0)
                self.wide += ok
                self.narrow += not ok
            self.fe.write_ragged(slots, self.store, offsets, vals, [self.stride[s] for s in slots])
        for s, n in sizes.items():
            self.at[s] += n


def same_packets(a, b):
    assert sorted(a) == sorted(b)
    for s in a:
        assert len(a[s]) == len(b[s])
        for x, y in zip(a[s], b[s]):
            assert [m for m, _ in x] == [m for m, _ in y], f"stream {s}: block sequence differs"
            for i, ((_, p), (_, q)) in enumerate(zip(x, y)):
                assert np.array_equal(np.frombuffer(p, np.uint8), np.frombuffer(q, np.uint8)), f"stream {s}: packet {i} differs"


@pytest.mark.parametrize("cls", [STEREO_Q5, MONO_8, SURROUND], ids=lambda c: IDS[c])
def test_mixed_sizes_in_one_step(oracle, cuda, cls):
    signals, schedule, want = mixed_case(oracle, cls)
    need_types(cls, want)
    assert any(len(step[1]) == 1 for step in schedule if step[0] == "write")
    assert any(len(step[1]) == NS for step in schedule if step[0] == "write")
    run = RaggedRun(cuda, cls, signals)
    got = run.run(signals, schedule)
    assert run.wide >= 3 and run.narrow >= 3, (run.wide, run.narrow)     # both copy paths ran
    run.fe.device_stats()
    assert run.fe.refused_writes == 0
    compare_slots(got, want, "ragged")
    run.close()


def test_against_the_grouped_path(oracle, cuda):
    """the same schedule through write_streams, once per distinct size, on a second front end"""
    cls = STEREO_Q5
    signals, schedule, _ = mixed_case(oracle, cls)
    ragged = RaggedRun(cuda, cls, signals)
    grouped = DeviceRun(cuda, cls, NS, "streams")
    same_packets(ragged.run(signals, schedule), grouped.run(signals, schedule))
    ragged.close()
    grouped.close()


def test_refused_calls_change_no_stream(oracle, cuda):
    """every refused call lists a stream that could take its samples next to the reason for the refusal: the run with
    the refused calls gives the packets of the run without them (and the oracle's)"""
    cls = STEREO_Q5
    signals, schedule, want = mixed_case(oracle, cls)
    plain = RaggedRun(cuda, cls, signals)
    run = RaggedRun(cuda, cls, signals)
    v, fe, store = run.v, run.fe, run.store
    cap = fe.capacity
    assert store.numel() >= cls[0] * cap + 64
    EINVAL = "code -131"                                             # VBM_EINVAL

    def refused(ids, offsets, vals, strides=None):
        before = fe.max_buffered
        with pytest.raises(v.VbmError, match=EINVAL):
            fe.write_ragged(ids, store, offsets, vals, strides)
        assert fe.max_buffered == before

    def refusals(finished):
        refused([1, 0, 1], [0, 0, 0], [64, 64, 64])                  # a duplicate id
        refused([0, NS], [0, 0], [64, 64])                           # ids out of range
        refused([0, -1], [0, 0], [64, 64])
        refused([0, 1], [0, 0], [64, 0])                             # vals == 0
        refused([0, 1], [0, 0], [64, 65], [64, 64])                  # ch_stride < vals
        refused([0, 1], [0, 0], [64, cap])                           # one stream of the list over capacity
        if finished:
            refused([0, NS - 1], [0, 0], [64, 64])                   # a write after finish

    cut = next(k for k, step in enumerate(schedule) if step[0] == "finish") + 2      # just after the early end's write
    run.run(signals, schedule[:3])
    refusals(False)                                                  # between a write and its drain
    run.run(signals, schedule[3:cut])
    refusals(True)
    got = run.run(signals, schedule[cut:])
    with pytest.raises(v.VbmError, match=EINVAL):                    # all ended
        fe.write_ragged([0], store, [0], [64])
    assert int(v.lib.vbm_frontend_write_ragged(fe._h, None, 0, None, None, None, None, None)) == 0   # nothing listed
    same_packets(got, plain.run(signals, schedule))
    compare_slots(got, want, "after refused calls")
    run.fe.device_stats()
    assert run.fe.refused_writes == 0
    run.close()
    plain.close()
