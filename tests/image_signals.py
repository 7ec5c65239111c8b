"""PCM whose channels are copies, negatives or near-copies of one another (numpy only, deterministic, at most 2 s each):
dual mono, polarity-flipped pairs, mono with a trace of side signal, a gain-only pan, one dead channel.  Every other
parity signal of the suite gives each channel its own harmonic, phase and noise; these drive couple/quantise onto its
exact ties instead: `abs(A) > abs(B)` with A = +-B in lossless_coupling / lossless_couplingf, `a > -b` with a = -b in
min_indemnity_dipole_hypot, an M6 residue_def of exactly 0, equal nepeak values handed from the angle to the magnitude
channel, and an angle vector that is all zero or -2 |magnitude| in every bin (oracle/orc_psy.c,
orc_couple_quantize_normalize).

Every signal is built from one burst_signal base (seed BASE_SEED, a burst every 20000 samples), so every stream still
switches blocks.  M is the base's channel 0 and S its channel 1.

tests/test_images_cpu.py holds the corpus to what it is for on the oracle alone; tests/test_images_gpu.py compares the
device with the oracle on all of it.  IMAGES is the corpus: one entry per (image, class)."""
import os
import sys

import numpy as np

from tests.reach_signals import entry, nsamples
from tests.signals import burst_signal

BASE_SEED = 3
BASE_PERIOD = 20000
SECONDS = 2.0


def base(ch, rate, seconds=SECONDS, seed=BASE_SEED):
    """the independent base: max(ch, 2) burst_signal channels, whole 1024-sample writes"""
    return burst_signal(max(ch, 2), rate, nsamples(rate, seconds), seed=seed, period=BASE_PERIOD)


def side_gain(db):
    """the float32 of 10^(-dB/20)"""
    return np.float32(10.0 ** (-db / 20.0))


# ---- two channels -------------------------------------------------------------------------------------------------------
def dual_mono(ch, rate):
    """(M, M): the two spectra are bit-identical, A = B in every lossless-coupled bin, the angle vector is zero"""
    b = base(2, rate)
    return np.stack([b[0], b[0]])


def inverted(ch, rate):
    """(M, -M): A = -B; lossless coupling leaves an angle of 2 |A|, which its last rule (`Ang >= 2 |Mag|`) turns into
    -2 |mag| in every bin that is not point-coupled away"""
    b = base(2, rate)
    return np.stack([b[0], -b[0]])


def near_mono(db):
    def make(ch, rate):
        """(M + g S, M - g S) in float32 arithmetic, g = side_gain(db): mono with a trace of side signal"""
        b = base(2, rate)
        g = side_gain(db)
        return np.stack([b[0] + g * b[1], b[0] - g * b[1]]).astype(np.float32)
    return make


def gain_pan(ch, rate):
    """(M, 0.5 M): a gain-only pan; the ratio is exact in float32, the spectra are not (the MDCT rounds)"""
    b = base(2, rate)
    return np.stack([b[0], np.float32(0.5) * b[0]])


def delay1(ch, rate):
    """(M, M one sample late)"""
    b = base(2, rate)
    return np.stack([b[0], np.concatenate([np.zeros(1, np.float32), b[0][:-1]])])


def hard_left(ch, rate):
    """(M, 0): the angle channel has no floor in any block"""
    b = base(2, rate)
    return np.stack([b[0], np.zeros_like(b[0])])


def hard_left_dither(ch, rate):
    """(M, 1e-6 S): an angle channel at -120 dB"""
    b = base(2, rate)
    return np.stack([b[0], np.float32(1e-6) * b[1]])


def swap_mid_stream(ch, rate):
    """(M, M) for the first half, then (M, -M): side_resdef and the block-to-block state cross the change"""
    b = base(2, rate)
    half = b.shape[1] // 2
    right = b[0].copy()
    right[half:] = -right[half:]
    return np.stack([b[0], right])


# ---- more than two channels -------------------------------------------------------------------------------------------
def all_same(ch, rate):
    b = base(ch, rate)
    return np.stack([b[0]] * ch)


def alt_sign(ch, rate):
    """(M, -M, M, -M, ..): which coupling steps pair equal and which opposite channels depends on the setup's pairs"""
    b = base(ch, rate)
    return np.stack([b[0] if c % 2 == 0 else -b[0] for c in range(ch)])


def one_live(ch, rate):
    b = base(ch, rate)
    x = np.zeros((ch, b.shape[1]), np.float32)
    x[0] = b[0]
    return x


def coupling_steps(ch, rate, q=None, bitrate=None):
    """[(magnitude channel, angle channel)] of the class, read from its mode pack (the long and the short map of every
    shipped pack couple the same pairs; this returns map 0's)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tools = os.path.join(root, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import vpk
    from tests.orc import mode_pack_name
    d = vpk.read_vpk(os.path.join(root, "vorbis_aotuv_lancer_amd", "data", mode_pack_name(ch, rate, q, bitrate)))
    n = int(d["map/0/coupling_steps"][0])
    return [(int(d["map/0/coupling_mag"][k]), int(d["map/0/coupling_ang"][k])) for k in range(n)]


def head(make, seconds):
    """the first `seconds` of an image (whole 1024-sample writes)"""
    return lambda ch, rate: np.ascontiguousarray(make(ch, rate)[:, :nsamples(rate, seconds)])


def front_same_rest_independent(q=None, bitrate=None):
    def make(ch, rate):
        """the two channels of the setup's first coupling step carry M, every other channel its own base channel: a
        tied step whose magnitude channel then meets independent channels in the later steps"""
        b = base(ch, rate)
        mag, ang = coupling_steps(ch, rate, q, bitrate)[0]
        x = b.copy()
        x[mag] = b[0]
        x[ang] = b[0]
        return x
    return make


# ---- the corpus -------------------------------------------------------------------------------------------------------
STEREO_ALL = [("dual_mono", dual_mono), ("inverted", inverted), ("near_mono_40", near_mono(40)),
              ("near_mono_80", near_mono(80)), ("near_mono_120", near_mono(120)), ("gain_pan", gain_pan),
              ("delay1", delay1), ("hard_left", hard_left), ("hard_left_dither", hard_left_dither),
              ("swap_mid_stream", swap_mid_stream)]
_S = dict(STEREO_ALL)
LADDER = ["dual_mono", "inverted", "near_mono_40", "near_mono_80"]       # in every stereo class
MINMAX = (144000, 128000, 112000)

# (rate, q, bitrate, the images beside LADDER): 2ch 44100 q0.5 has all ten, every other class six
STEREO_CLASSES = [
    (44100, 0.5, None, [n for n, _ in STEREO_ALL if n not in LADDER]),
    (44100, 0.1, None, ["gain_pan", "hard_left_dither"]),
    (44100, 1.0, None, ["near_mono_120", "delay1"]),
    (44100, -0.1, None, ["swap_mid_stream", "hard_left"]),              # 512 / 4096
    (22050, 0.5, None, ["gain_pan", "swap_mid_stream"]),                # 512 / 1024, 8-bin partitions in both block sizes
    (96000, 0.5, None, ["delay1", "hard_left_dither"]),
    (44100, None, 128000, ["swap_mid_stream", "gain_pan"]),
    (44100, None, MINMAX, ["swap_mid_stream", "hard_left"]),
]
# (rate, q, bitrate, seconds): managed 5.1 walks its fifteen blobs through the serial couple kernel one after the other,
# ten times the device time per block of any other class here, so its streams are the first half second
COUPLED_6 = [(48000, 0.3, None, SECONDS), (48000, 0.1, None, SECONDS), (48000, None, 320000, 0.5)]
UNCOUPLED = [(6, 48000, 0.8), (3, 44100, 0.5), (5, 44100, 0.5), (8, 44100, 0.5)]

IMAGES = []
for _rate, _q, _br, _more in STEREO_CLASSES:
    IMAGES += [entry(n, _S[n], 2, _rate, _q, _br) for n in LADDER + _more]
for _rate, _q, _br, _secs in COUPLED_6:
    IMAGES += [entry("all_same", head(all_same, _secs), 6, _rate, _q, _br),
               entry("alt_sign", head(alt_sign, _secs), 6, _rate, _q, _br),
               entry("front_same_rest_independent", head(front_same_rest_independent(_q, _br), _secs), 6, _rate, _q, _br),
               entry("one_live", head(one_live, _secs), 6, _rate, _q, _br)]
    for _e in IMAGES[-4:]:
        _e["seconds"] = _secs
IMAGES += [entry("all_same", all_same, _ch, _rate, _q) for _ch, _rate, _q in UNCOUPLED]
for _e in IMAGES:
    _e.setdefault("seconds", SECONDS)


def class_of(e):
    return (e["ch"], e["rate"], e["q"], e["bitrate"])


def classes():
    """the corpus' classes, in order of first appearance"""
    out = []
    for e in IMAGES:
        if class_of(e) not in out:
            out.append(class_of(e))
    return out


def images_of(ch, rate, q=None, bitrate=None):
    return [e for e in IMAGES if class_of(e) == (ch, rate, q, bitrate)]


def seconds_of(ch, rate, q=None, bitrate=None):
    """the length of the class's streams (one length per class)"""
    return images_of(ch, rate, q, bitrate)[0]["seconds"]
