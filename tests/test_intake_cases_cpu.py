"""The intake cases of tests/intake_cases.py have teeth: checked on the oracle alone, without a GPU.

These are conditions on the INPUTS of tests/test_intake_gpu.py, not on the product: if a recipe change breaks one,
the recipe changes, not the condition."""
import pytest

from tests import intake_cases as ic
from tests import orc


@pytest.fixture(scope="module")
def setups(oracle):
    return {cls: orc.Setup(oracle, *cls) for cls in ic.CLASSES}


def one_stream(oracle, setup, sig, schedule):
    return ic.oracle_run(oracle, setup, {0: sig}, schedule)[0][0]


@pytest.mark.parametrize("cls", ic.CLASSES, ids=lambda c: f"{c[0]}ch-{c[1]}-q{c[2]:g}")
def test_write_size_changes_the_first_packet_only(oracle, setups, cls):
    """_preextrapolate_helper runs at the write that first takes the stream past one long block (lib/block.c:547-550)
    and fits to everything written so far: the first packet differs from the 1024-sample schedule's exactly when the
    total written at that moment differs; all later packets and the packet count are the same."""
    setup = setups[cls]
    bs1 = ic.blocksizes(setup)[1]
    runs = {}
    for name in ["1024"] + ic.SCHEDULE_NAMES:
        total = ic.write_samples(name, bs1)
        sig = ic.write_signals(cls[0], cls[1], total, 1)[0]
        key = (name, total)
        runs[key] = (ic.size_list(name, bs1, total), one_stream(oracle, setup, sig, ic.write_size_schedule(name, bs1, [0], total)))
        if ("1024", total) not in runs:
            runs[("1024", total)] = (ic.size_list("1024", bs1, total),
                                     one_stream(oracle, setup, sig, ic.write_size_schedule("1024", bs1, [0], total)))
    differing = 0
    for (name, total), (sizes, seq) in runs.items():
        base_sizes, base = runs[("1024", total)]
        assert len(seq) == len(base) and len(seq) > 4, (name, len(seq), len(base))
        assert seq[1:] == base[1:], f"{name}: a packet after the first differs from the 1024-sample schedule"
        assert seq[-1][0][4] == 1
        same_crossing = ic.crossing_total(sizes, bs1) == ic.crossing_total(base_sizes, bs1)
        assert (seq[0] == base[0]) == same_crossing, (name, ic.crossing_total(sizes, bs1), ic.crossing_total(base_sizes, bs1))
        differing += not same_crossing
    assert differing >= 10, differing


def test_second_write_signal_depends_on_the_write_size_beyond_the_first_packet(oracle, setups):
    """the recipe of stream 1: the delivery reaches past the first packet (how far ahead the envelope marks are known
    when a block is carved), so the device has to follow the oracle there too"""
    cls = (2, 44100, 0.5)
    bs1 = ic.blocksizes(setups[cls])[1]
    sig = ic.write_signals(cls[0], cls[1], ic.WRITE_SAMPLES)[1]
    base = one_stream(oracle, setups[cls], sig, ic.write_size_schedule("1024", bs1, [0], ic.WRITE_SAMPLES))
    later = [name for name in ic.SCHEDULE_NAMES if name != "largest" and
             one_stream(oracle, setups[cls], sig, ic.write_size_schedule(name, bs1, [0], ic.WRITE_SAMPLES))[1:] != base[1:]]
    assert later, "no schedule changes a packet after the first"


def test_one_sample_writes_cross_one_sample_past_the_long_block(oracle, setups):
    cls = (2, 22050, 0.5)
    bs1 = ic.blocksizes(setups[cls])[1]
    assert ic.crossing_total([1] * (bs1 + 300), bs1) == bs1 + 1


def short_blocks(seq):
    return sum(1 for m, _ in seq if m[1] == 0)


def test_onset_offset_sweep_moves_the_block_boundaries(oracle, setups):
    cls = (2, 44100, 0.5)
    seqs = []
    for onset in ic.ONSET_OFFSETS:
        sig = ic.onset_signal(cls[0], cls[1], onset=onset)
        seq = one_stream(oracle, setups[cls], sig, ic.lockstep_schedule([sig.shape[1]]))
        assert short_blocks(seq) > 0, onset
        seqs.append(tuple(m[:4] for m, _ in seq))
    assert len(set(seqs)) >= 2, len(set(seqs))


@pytest.mark.parametrize("cls", [(2, 44100, 0.5), (2, 22050, 0.5)], ids=["44100", "22050"])
def test_onset_amplitude_sweep_crosses_the_trigger(oracle, setups, cls):
    counts = []
    for amp in ic.ONSET_AMPS:
        sig = ic.onset_signal(cls[0], cls[1], amp=amp)
        counts.append(short_blocks(one_stream(oracle, setups[cls], sig, ic.lockstep_schedule([sig.shape[1]]))))
    assert len(set(counts)) >= 2, counts
    assert counts[-1] > counts[0], counts


@pytest.mark.parametrize("cls", ic.CLASSES, ids=lambda c: f"{c[0]}ch-{c[1]}-q{c[2]:g}")
@pytest.mark.parametrize("drain_as_you_go", [True, False])
def test_edge_lengths_all_yield_packets(oracle, setups, cls, drain_as_you_go):
    setup = setups[cls]
    lengths = ic.edge_lengths(ic.blocksizes(setup)[1])
    sigs = ic.edge_signals(cls[0], cls[1], lengths)
    want = ic.oracle_run(oracle, setup, sigs, ic.edge_length_schedule(lengths, drain_as_you_go))
    for s, L in enumerate(lengths):
        seq = want[s][0]
        assert len(seq) >= 1, L
        assert seq[-1][0][4] == 1 and all(m[4] == 0 for m, _ in seq[:-1]), L
        assert seq[-1][0][5] == L, (L, seq[-1][0][5])      # the last granule position is the sample count
