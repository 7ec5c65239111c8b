"""The edge signals of tests/test_vq_edges_gpu.py (numpy only: tools/oracle_reach.py draws them too)."""
import numpy as np

from tests.signals import synth_signal

N = 44100 * 3 // 2          # 1.5 s: start of the stream, long blocks, two bursts of short blocks


def one_silent(ch, rate):
    x = synth_signal(ch, rate, N, seed=21)
    x[1] = 0.0
    return x


def both_silent_for_a_while(ch, rate):
    x = synth_signal(ch, rate, N, seed=22)
    x[:, N // 3:2 * N // 3] = 0.0
    return x


def square(ch, rate):
    """full scale, a period that is no divisor of a block, a different phase per channel"""
    t = np.arange(N)
    return np.stack([np.where(((t + 37 * c) // 45) % 2 == 0, 1.0, -1.0) for c in range(ch)]).astype(np.float32)


def clipped_noise(ch, rate):
    rng = np.random.default_rng(23)
    x = np.clip(4.0 * rng.standard_normal((ch, N)), -1.0, 1.0)
    x[:, N // 2:] *= np.where(np.arange(N - N // 2) % 9000 < 4500, 1.0, 0.02)      # loud / quiet: block switching
    return x.astype(np.float32)


def surround(ch, rate):
    x = synth_signal(ch, rate, N, seed=24)
    x[3] = 0.0                                  # one channel of a coupled submap silent
    x[5, : N // 2] = 0.0                        # the LFE's own submap empty for half of the signal
    return x


CASES = [
    ("one_silent", 2, 44100, 0.5, one_silent),
    ("both_silent_for_a_while", 2, 44100, 0.5, both_silent_for_a_while),
    ("square_q0.1_stereo", 2, 44100, 0.1, square),
    ("square_q1_stereo", 2, 44100, 1.0, square),
    ("square_q0.1_mono", 1, 44100, 0.1, square),
    ("square_q1_mono", 1, 44100, 1.0, square),
    ("clipped_noise_q0.1_stereo", 2, 44100, 0.1, clipped_noise),
    ("clipped_noise_q1_stereo", 2, 44100, 1.0, clipped_noise),
    ("clipped_noise_q0.1_mono", 1, 44100, 0.1, clipped_noise),
    ("clipped_noise_q1_mono", 1, 44100, 1.0, clipped_noise),
    ("surround_5.1", 6, 48000, 0.5, surround),
]
