"""k_fe_ve_filter (the envelope detector's filter walk) where its spreading step can go wrong: block sequence (types,
window flags, granule positions, packet numbers) and packets of whole streams from raw PCM, against the oracle.

The spreading step compares each of the 32 smoothed spectrum values with the near-DC `decay` after k subtractions of
8 (value k), each subtraction rounded to float as the source does.  A lane owns values jb and jb + 16 and takes the
chain's value at those two points.

  streams   1, 3 and 5: four streams share a wavefront, so a lone group, a part-filled one and a second workgroup
  channels  1 and 2
  writes    64, 512 and 2112 samples, drained after every write: 1, 8 and 33 search steps (of 64 samples) per
            evaluation; 33 needs a second launch of the VBM_FE_CHUNK = 32 step kernels
  signals   a strong tone below 100 Hz at levels 1e-4 .. 1 (one level per stream, rotating with the case so that the
            one-stream cases cover them all) with a noise burst, so that marks are set and short blocks come.
            `decay` is 10 log10 of the near-DC energy less 15 dB: between about -65 and +15 over these levels, and the
            chain goes 248 below its start, so it crosses the magnitudes 16, 32, 64 and 128 (32 upward only from
            the lowest levels on) — where the float spacing changes and a subtraction of 8 has to round — while the
            spectrum values it is compared with lie in the same range."""
import numpy as np
import pytest

from tests.encode_calls import write_and_drain
from tests.encode_oracle import RECORD_KEEP, compare_records, records, walk

NSAMP, BURST = 13 * 1024, 7300
LEVELS = (1e-4, 1e-3, 1e-2, 0.1, 1.0)
FREQS = (31.0, 47.0, 63.0, 79.0, 95.0)
CASES = [(S, ch, W) for S in (1, 3, 5) for ch in (1, 2) for W in (64, 512, 2112)]


def low_tone(ch, rate, level, f, seed):
    rng = np.random.default_rng(seed)
    pos = np.arange(NSAMP)
    t = pos / rate
    burst = (pos >= BURST) & (pos < BURST + 200)
    out = np.empty((ch, NSAMP), np.float32)
    for c in range(ch):
        x = 0.9 * level * np.sin(2 * np.pi * f * (1.0 + 0.11 * c) * t + c)
        x += np.where(burst, min(1.0, 40.0 * level) * 0.6 * rng.uniform(-1, 1, NSAMP), 0.0)
        out[c] = x.astype(np.float32)
    return out


def case_signals(S, ch, W):
    rot = CASES.index((S, ch, W))
    return [low_tone(ch, 44100, LEVELS[(s + rot) % 5], FREQS[(s + 2 * rot) % 5], seed=900 + 7 * rot + s) for s in range(S)]


def oracle_streams(oracle, S, ch, W):
    """the oracle fed the same writes (W samples, drained after every write, then end of stream): computed once"""
    return [records(walk(oracle, ch, 44100, 0.5, pcm=sig, chunk=W, capture=False, keep=RECORD_KEEP, key=("envelope", S, W, s)))
            for s, sig in enumerate(case_signals(S, ch, W))]


def test_every_level_is_used_by_a_one_stream_case():
    used = {LEVELS[CASES.index(c) % 5] for c in CASES if c[0] == 1}
    assert used == set(LEVELS)


@pytest.mark.parametrize("S,ch,W", CASES)
def test_oracle_switches_blocks_in_every_case(oracle, S, ch, W):
    """(CPU) every stream of every case has long and short blocks by the oracle alone: marks were set"""
    for s, seq in enumerate(oracle_streams(oracle, S, ch, W)):
        sizes = {m[1] for m, _ in seq}
        assert sizes == {0, 1}, (s, sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("S,ch,W", CASES)
def test_block_sequence_and_packets(oracle, cuda, S, ch, W):
    import vorbis_aotuv_lancer_amd as v
    want = oracle_streams(oracle, S, ch, W)
    setup = v.Setup(ch, 44100, 0.5)
    enc = v.Encoder(setup, S)
    fe = v.FrontEnd(enc)
    try:
        got = [[] for _ in range(S)]
        write_and_drain(fe, cuda, case_signals(S, ch, W), got, chunk=W)
        for s in range(S):
            compare_records(got[s], want[s], f"stream {s}")
    finally:
        fe.close()
        enc.close()
        setup.close()
