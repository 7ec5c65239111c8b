"""What the live-store tests share (tests/test_live_store_cpu.py, tests/test_live_store_gpu.py): streams whose packets
are a head byte of tests/decode_packets.py's one-byte corpus with seeded bytes behind it, and the trim rule restated."""
import numpy as np


def padded(stream, rng, most):
    """the stream's one-byte packets with up to most - 1 seeded bytes behind each: the index stays what it is"""
    data, off, gp, eos = stream
    sizes = rng.integers(1, most + 1, len(off) - 1)
    out = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    o = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out[o[:-1]] = data
    return out, o, gp, eos


def drop_rule(sizes, np_, nb, MP, MB):
    """The rule restated.  sizes: the bytes of each retained packet; np_ packets of nb bytes arrive at capacities MP and
    MB.  Nothing is dropped while the run fits; else the fewest packets from the front such that what remains is at most
    half of each capacity and leaves the run its room."""
    if len(sizes) + np_ <= MP and sum(sizes) + nb <= MB:
        return 0
    d = 0
    while len(sizes) - d > min(MP // 2, MP - np_) or sum(sizes[d:]) > min(MB // 2, MB - nb):
        d += 1
    return d
