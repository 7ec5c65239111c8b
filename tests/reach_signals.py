"""PCM that drives the encoder down branches the synth_signal / burst_signal family never takes (numpy only,
deterministic, at most 2 s each).  Every docstring names the `/* REACH: name */` targets of oracle/*.c the signal is
for; tools/oracle_reach.py counts them, tests/test_reach_cpu.py holds each signal to what it is for, and
tests/test_reach_gpu.py compares the device with the oracle on all of them ("Oracle branches").

REACH is the corpus: one entry per (signal, class)."""
import numpy as np


def nsamples(rate, seconds):
    """whole 1024-sample writes, like the front-end tests feed their streams"""
    return int(seconds * rate) // 1024 * 1024


# amplitude of hit k (cycled): hits 0..2 are what the detector's value ranges need at 2ch 44100 q0.5 (below), the
# rest is the loud / medium / quiet cycle
HIT_AMPS = (0.5, 0.5, 0.5, 0.9, 0.08, 0.3, 0.9, 0.08, 0.3, 0.9)
CHANNEL_GAIN = (1.0, 0.8, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
SOLO_HIT = 3        # this hit sounds in channel 0 alone


def decaying_hits(ch, rate, seconds=2.0, seed=5, solo=SOLO_HIT):
    """Noise hits that decay exponentially into a 1e-4 noise bed: a percussive hit ringing out into quiet.

    Hit k starts 9000 + 211 (k mod 7) samples after hit k-1 (the first at 3000), is 8 tau long with
    tau = 120 + 23 k samples, and has amplitude HIT_AMPS[k mod 10] x CHANNEL_GAIN[channel]; hit `solo` is in channel 0
    only.  The envelope search answers each hit with impulse short blocks and leaves through a long transition block
    whose second quarter still holds the tail while the third is down at the bed: aoTuV's M2 post-echo detector
    (orc_postnoise_detection) returns a positive value there.

    REACH: poste_positive, poste_below_tenth, postecho_npeak_minus1, m8_skip_postecho, couple_npeak_minus1
    (at 2ch 44100 q0.5 hit 0 gives 0.135 in channel 0 and a value in (0, 0.1), turned into -1, in channel 1; hit 1
    gives values >= 30, where VMIN(poste, 30) acts; hit 2 values in [0.1, 30); hit 3 a positive value in channel 0 next
    to a channel that fails on its loud quarter)."""
    n = nsamples(rate, seconds)
    x = 1e-4 * np.random.default_rng([seed, 1000]).uniform(-1, 1, (ch, n))
    at, k = 3000, 0
    while at < n:
        tau = 120 + 23 * k
        length = min(8 * tau, n - at)
        hit = HIT_AMPS[k % len(HIT_AMPS)] * np.random.default_rng([seed, k]).uniform(-1, 1, length)
        hit *= np.exp(-np.arange(length) / tau)
        for c in range(ch if k != solo else 1):
            x[c, at:at + length] += CHANNEL_GAIN[c] * hit
        at += 9000 + 211 * (k % 7)
        k += 1
    return x.astype(np.float32)


def click_trains(ch, rate, seconds=2.0, seed=6):
    """Three-sample clicks on a 1e-4 noise bed: 0.45 s of dense clicks (one every 300 samples: impulse short blocks in
    a row, lW_no >= 4), then pairs of clicks 700, 1100, 1500 .. samples apart (impulse, padding, impulse again:
    impadnum set when the second impulse block is analysed), each pair followed by quiet.

    REACH: m3p256_lwno_ge4, m3p256_impadnum (with m3p256_lwno_lt4 and m3p256_after_padding, which the suite takes
    already) in the one shipped class whose short block is 512 at 26 kHz and more, 2ch 44100 q-0.1; m3p128_impadnum and
    the same block orders at n = 128; at 1ch 8000, n = 256 below 26 kHz, set_m3p returns before its switch."""
    n = nsamples(rate, seconds)
    rng = np.random.default_rng(seed)
    x = 1e-4 * rng.uniform(-1, 1, (ch, n))
    at = [2000 + 300 * i for i in range(int(0.45 * rate) // 300)]
    t, gap = at[-1] + 6000, 700
    while t + gap + 3 < n:
        at += [t, t + gap]
        t += gap + 5000
        gap += 400
    for k, a in enumerate(at):
        for c in range(ch):
            x[c, a:a + 3] += (0.9, -0.7, 0.4) if (k + c) % 2 else (-0.8, 0.6, -0.3)
    return x.astype(np.float32)


def faint_noise(ch, rate, seconds=2.0, seed=7):
    """Noise at 1e-9, 1e-7 and 1e-5 in turn (a third of the signal each) with one 0.5 click in every third: spectra
    whose noise estimate lies below 0 dB on the encoder's scale, in long and in short blocks.

    REACH: interpolate_fit_missing_neighbour, floor_fit_both_degenerate (2ch 44100 b256000: at these levels a block
    has a floor at the middle rate and none at the high or the low one, so the interpolated fits of the packetblobs in
    between come out empty), compand_db_below0 (compand_low_db_below0, the same clamp in the loop that runs while the loud-noise fix
    holds a positive level, was searched for with this and with the hits on low-passed beds and was not reached)"""
    n = nsamples(rate, seconds)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (ch, n))
    third = n // 3
    for k, a in enumerate((1e-9, 1e-7, 1e-5)):
        x[:, k * third:(k + 1) * third if k < 2 else n] *= a
        x[:, k * third + third // 2: k * third + third // 2 + 3] = 0.5
    return x.astype(np.float32)


def gated_bands(ch, rate, seconds=2.0, seed=8):
    """Band-limited tone clusters (a few exact sines, no noise at all) gated on and off in 4096-sample segments, with
    digital zero in a third of every channel's segments, at different times in different channels: blocks in which the
    magnitude channel of a coupled pair has no floor while its angle channel has one (`nz[Mi]` clear, `nz[Ai]` set in
    orc_couple_quantize_normalize: a direction of an `||`, with no line of its own to tag; the suite's one-sided
    silence is always in the angle channel), and lossless coupling of 0 with 0, the one case in which
    `*Ang >= 2 |*Mag|` holds.

    REACH: point_coupling_multi_step (6ch 48000 q0.1)"""
    n = nsamples(rate, seconds)
    t = np.arange(n) / rate
    rng = np.random.default_rng(seed)
    x = np.zeros((ch, n))
    nseg = n // 4096
    for c in range(ch):
        for s in range(nseg):
            if (s + c) % 3 == 2:
                continue                                                    # digital zero
            f0 = rate * (0.01, 0.11, 0.23, 0.37, 0.45)[(s + 2 * c) % 5]
            seg = slice(s * 4096, (s + 1) * 4096)
            for h in range(1 + s % 3):
                x[c, seg] += (0.4 / (1 + h)) * np.sin(2 * np.pi * (f0 + 31.0 * h) * t[seg] + rng.uniform(0, 6))
    return x.astype(np.float32)


def edge_tones(ch, rate, seconds=2.0, seed=9):
    """A sweep from 5 Hz to Nyquist, a tone 0.2 bins above DC, a tone half a bin below Nyquist and the alternating
    sequence +a, -a (Nyquist itself), a third of the signal each, with a click at each seam: energy in the first and
    the last bins of the spectrum.

    REACH: none by name.  The signal was written for the early exits of the bark-noise window loops and for
    ntfix_nxplus_over_n; both turned out to depend on the setup's tables alone.  It stays as a parity
    input of a kind the other families lack."""
    n = nsamples(rate, seconds)
    t = np.arange(n) / rate
    third = n // 3
    sweep = 0.5 * np.sin(2 * np.pi * (5.0 * t + (rate / 2 - 5.0) / (2 * third / rate) * t * t))
    low = 0.6 * np.sin(2 * np.pi * (0.2 * rate / 2048) * t)
    high = 0.5 * np.sin(2 * np.pi * (rate / 2 - 0.5 * rate / 2048) * t)
    alt = 0.4 * np.where(np.arange(n) % 2, -1.0, 1.0)
    x = np.zeros((ch, n))
    for c in range(ch):
        x[c, :third] = sweep[:third] if c % 2 == 0 else sweep[:third][::-1]
        x[c, third:2 * third] = low[third:2 * third] + (high[third:2 * third] if c % 2 else 0.0)
        x[c, 2 * third:] = np.where(t[2 * third:] < t[2 * third] + 0.25, high[2 * third:], alt[2 * third:])
        x[c, third:third + 3] += 0.4
        x[c, 2 * third:2 * third + 3] -= 0.4
    return x.astype(np.float32)


def zero_tail(ch, rate, seconds=2.0, seed=10):
    """Digital zero for 0.6 s, a tone on noise for 0.6 s, then digital zero to the end: the start-of-stream and the
    end-of-stream extrapolation both fit their predictor to a zero-energy buffer.

    REACH: lpc_error_below_epsilon (the suite's silent streams take it too; here it comes after content, so the
    predictor runs over a buffer that is zero only in its fitted part)"""
    n = nsamples(rate, seconds)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = np.stack([0.3 * np.sin(2 * np.pi * 440.0 * (c + 1) * t) + 0.05 * rng.uniform(-1, 1, n) for c in range(ch)])
    x[:, :int(0.6 * rate)] = 0.0
    x[:, int(1.2 * rate):] = 0.0
    return x.astype(np.float32)


def overdriven_noise(ch, rate, seconds=2.0, seed=11):
    """Gaussian noise at 0.01 with 0.4 s of it at 30 times full scale from 0.5 s and from 1.3 s on: float PCM is not bounded by 1, and at the lowest quality
    the fitted floor line then leaves the top of the floor's range.

    REACH: fitline_y0_above_1023 (2ch 44100 q-0.1), bitrate_truncates_packet (2ch 44100 b128000 with a maximum of
    144000: even packetblob 0 overshoots what the reservoir can take, and the packet is cut)"""
    n = nsamples(rate, seconds)
    x = np.random.default_rng(seed).standard_normal((ch, n))
    x *= 0.01
    for at in (0.5, 1.3):
        x[:, int(at * rate):int((at + 0.4) * rate)] *= 3000.0
    return x.astype(np.float32)


def entry(name, make, ch, rate, q=None, bitrate=None):
    if bitrate is None:
        tail = f"q{q:g}"
    else:
        tail = f"b{bitrate}" if isinstance(bitrate, int) else f"b{bitrate[1]}_max{bitrate[0]}_min{bitrate[2]}"
    return dict(name=f"{name}_{ch}ch_{rate}_{tail}", make=make, ch=ch, rate=rate, q=q, bitrate=bitrate)


REACH = [
    entry("decaying_hits", decaying_hits, 2, 44100, 0.5),
    entry("decaying_hits", decaying_hits, 1, 44100, 0.1),
    entry("decaying_hits", decaying_hits, 6, 48000, 0.3),          # coupled 5.1
    entry("decaying_hits", decaying_hits, 2, 44100, -0.1),         # long block 4096, short block 512
    entry("decaying_hits", decaying_hits, 2, 22050, 0.5),          # long block 1024: the detector returns -1 throughout
    entry("decaying_hits", decaying_hits, 2, 44100, bitrate=128000),
    entry("click_trains", click_trains, 2, 44100, -0.1),           # n = 256 short blocks at 44.1 kHz
    entry("click_trains", click_trains, 1, 8000, 0.5),             # n = 256 blocks below 26 kHz: no M3 at all
    entry("click_trains", click_trains, 2, 44100, 0.5),
    entry("faint_noise", faint_noise, 2, 44100, 0.5),
    entry("faint_noise", faint_noise, 2, 44100, bitrate=256000),   # managed: the mid-rate fit exists, a neighbour does not
    entry("gated_bands", gated_bands, 2, 44100, 0.5),
    entry("gated_bands", gated_bands, 6, 48000, 0.1),              # lower-quality 5.1: multi-step point coupling
    entry("edge_tones", edge_tones, 2, 44100, 0.5),
    entry("zero_tail", zero_tail, 2, 44100, 0.5),
    entry("overdriven_noise", overdriven_noise, 2, 44100, -0.1),
    entry("overdriven_noise", overdriven_noise, 2, 44100, bitrate=(144000, 128000, 112000)),   # past the maximum rate
]
