"""plan_files on the oracle alone: the schedule that drives slots through a list of files gives every file the packets
it has when it is encoded alone by the reference application's loop, whatever the slot count."""
import pytest

from tests import encode_files_cases as fc
from tests import intake_cases as ic

STEREO_Q5, MONO_8 = (2, 44100, 0.5), (1, 8000, 0.5)


def check_plan(schedule, files, lengths, nslots, chunk=1024):
    """the schedule's own shape, without any encoder"""
    S = min(nslots, len(lengths))
    assert len(files) == S
    # every file lives in exactly one (slot, generation), taken in list order
    assert sorted(f for gens in files for f in gens) == list(range(len(lengths)))
    assert [gens[0] for gens in files] == list(range(S))
    gen, written, state = [0] * S, [0] * S, ["open"] * S            # open -> finished -> (restart) open
    order = list(range(S))
    for k, step in enumerate(schedule):
        if step[0] == "write":
            assert schedule[k + 1] == ("drain",)
            for s, n in step[1].items():
                assert state[s] == "open", "a write to a finished stream"
                L = lengths[files[s][gen[s]]]
                assert n == min(chunk, L - written[s]) and n > 0
                written[s] += n
        elif step[0] == "finish":
            assert schedule[k - 1][0] in ("drain", "restart") if k else True      # the stream is drained by then
            assert schedule[k + 1][0] in ("write", "drain")
            for s in step[1]:
                assert state[s] == "open" and written[s] == lengths[files[s][gen[s]]]
                state[s] = "finished"
        elif step[0] == "restart":
            assert schedule[k - 1] == ("drain",)
            for s in step[1]:
                assert state[s] == "finished"
                gen[s] += 1
                written[s], state[s] = 0, "open"
                order.append(files[s][gen[s]])
        else:
            assert step == ("drain",)
            # every open slot has either written in this step or is finished: a slot never idles between its writes
            back = k - 1
            named = set()
            while back >= 0 and schedule[back][0] in ("write", "finish"):
                named |= set(schedule[back][1])
                back -= 1
            assert named >= {s for s in range(S) if state[s] == "open"}
    assert state == ["finished"] * S and [g + 1 for g in gen] == [len(gens) for gens in files]
    assert order == list(range(len(lengths)))                       # the next file in list order


def run_plan(oracle, cls, lengths, signals, nslots):
    import vorbis_aotuv_lancer_amd as v
    schedule, files = v.plan_files(lengths, nslots)
    check_plan(schedule, files, lengths, nslots)
    per_slot = [[signals[f] for f in gens] for gens in files]
    got = ic.oracle_run(oracle, fc.osetup(oracle, cls), per_slot, schedule)
    want = fc.alone(oracle, cls, "edge", signals)
    for s, gens in enumerate(files):
        assert len(got[s]) == len(gens)
        for g, f in enumerate(gens):
            assert got[s][g] == want[f], f"file {f} ({lengths[f]} samples) in slot {s}.{g} differs from the file alone"


@pytest.mark.parametrize("nslots", [1, 3, 5, 18])
def test_every_file_as_if_alone(oracle, nslots):
    lengths, signals = fc.edge_files(oracle, STEREO_Q5)
    assert lengths == ic.edge_lengths(2048) + [12345, 30000] and nslots <= len(lengths)
    want = fc.alone(oracle, STEREO_Q5, "edge", signals)
    assert all(seq and seq[-1][0][4] == 1 for seq in want)           # every file ends in e_o_s, the empty one too
    assert {m[1] for seq in want[-2:] for m, _ in seq} == {0, 1}     # short and long blocks in the burst files
    run_plan(oracle, STEREO_Q5, lengths, signals, nslots)


def test_one_block_size(oracle):
    lengths, signals = fc.edge_files(oracle, MONO_8)
    run_plan(oracle, MONO_8, lengths, signals, 5)


def test_plan_of_nothing_and_of_bad_input():
    import vorbis_aotuv_lancer_amd as v
    assert v.plan_files([], 4) == ([], [])
    assert v.plan_files([0], 4) == ([("finish", [0]), ("drain",)], [[0]])
    assert v.plan_files([1500, 0], 1, chunk=1000) == (
        [("write", {0: 1000}), ("drain",), ("write", {0: 500}), ("drain",), ("finish", [0]), ("drain",),
         ("restart", [0]), ("finish", [0]), ("drain",)], [[0, 1]])
    for bad in (([-1], 1), ([5], 0)):
        with pytest.raises(ValueError):
            v.plan_files(*bad)


def test_unsupported_class_is_setups_error():
    import numpy as np
    import vorbis_aotuv_lancer_amd as v
    with pytest.raises(FileNotFoundError):
        v.encode_ogg([np.zeros((2, 10), np.float32)], 12345)
    assert v.encode_ogg([], 44100) == []
    for bad in ([np.zeros((2, 10), np.float64)], [np.zeros(10, np.float32)]):
        with pytest.raises(ValueError):
            v.encode_ogg(bad, 44100)
