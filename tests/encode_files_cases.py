"""File lists for the whole-file encode tests (numpy only), and what the oracle makes of each file on its own.

A file's reference is ONE oracle stream that is given the file as the reference application gives it
(examples/encoder_example.c:179-236): 1024 samples per write, a drain after each, the end in the step after the last
write, a drain — intake_cases.edge_length_schedule([L], True).  Computed once per (class, file list) and shared."""
from tests import intake_cases as ic
from tests import orc
from tests.signals import burst_signal

_setups, _alone = {}, {}


def osetup(oracle, cls):
    """cls: (channels, rate, quality) or (channels, rate, None, bitrate) for a managed pack"""
    if cls not in _setups:
        _setups[cls] = orc.Setup(oracle, *cls)
    return _setups[cls]


def edge_files(oracle, cls):
    """every edge length of the class (0, 1, 31..33, a long block +-1, three long blocks + 1, ...) with a signal that is
    loud from its first sample, then two longer files with bursts, so that short blocks occur -> (lengths, signals)"""
    bs1 = ic.blocksizes(osetup(oracle, cls))[1]
    edges = ic.edge_lengths(bs1)
    lengths = edges + [12345, 30000]
    signals = ic.edge_signals(cls[0], cls[1], edges)
    signals += [burst_signal(cls[0], cls[1], L, seed=910 + k) for k, L in enumerate(lengths[len(edges):])]
    return lengths, signals


def small_files(oracle, cls):
    """{0, 1, bs1 + 1, 3 bs1 + 1, 9000}: the last with bursts"""
    bs1 = ic.blocksizes(osetup(oracle, cls))[1]
    lengths = [0, 1, bs1 + 1, 3 * bs1 + 1, 9000]
    signals = ic.edge_signals(cls[0], cls[1], lengths[:4]) + [burst_signal(cls[0], cls[1], 9000, seed=930)]
    return lengths, signals


def alone(oracle, cls, key, signals):
    """[(info, packet) sequence of file i run alone]; info = (lW, W, nW, block type, e_o_s, granulepos, packetno)"""
    if (cls, key) not in _alone:
        setup = osetup(oracle, cls)
        _alone[(cls, key)] = [ic.oracle_run(oracle, setup, [sig], ic.edge_length_schedule([sig.shape[1]], True))[0][0]
                              for sig in signals]
    return _alone[(cls, key)]
