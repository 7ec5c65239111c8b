"""What tests/test_images_cpu.py and tests/test_images_gpu.py share on the correlated-channel corpus
(tests/image_signals.py): the oracle's blocks of an image, the decoder model's spectra of its packets, and the
copies-or-negatives relation of decoded rows."""
import functools

import numpy as np

from tests import vorbis_model as vm
from tests.decode_packets import unpack_headers
from tests.encode_oracle import walk
from tests.image_signals import base, images_of

_cache = {}


def cid(c):
    ch, rate, q, bitrate = c
    if bitrate is None:
        return f"{ch}ch_{rate}_q{q:g}"
    return f"{ch}ch_{rate}_b{bitrate}" if isinstance(bitrate, int) else "%dch_%d_b%d_max%d_min%d" % (ch, rate, bitrate[1], bitrate[0], bitrate[2])


def encode(oracle, key, c, make):
    """the oracle's blocks of the stream make(ch, rate), 1024 samples per write and the end of the stream declared:
    computed once"""
    ch, rate, q, bitrate = c

    def pcm():
        x = make(ch, rate)
        assert 0 < x.shape[1] <= 2 * rate and x.shape[1] % 1024 == 0
        return x
    return walk(oracle, ch, rate, q, bitrate, pcm, key=("images", key))


def blocks(oracle, c, image):
    e = next(e for e in images_of(*c) if e["name"].startswith(image + "_%dch" % c[0]))
    return encode(oracle, e["name"], c, e["make"])


def independent(oracle, c):
    """the class's independent base: what the images are made from, each channel on its own"""
    return encode(oracle, "base", c, base)


# ---- the decoder property the device test relies on -------------------------------------------------------------------
# (class, image, relation of the decoded rows).  Inverted at q1.0 keeps every pair lossless, so every non-zero bin
# decodes to exact negatives; at q0.5 the encoder point-couples 1855 magnitude values (angle 0), and a point-coupled bin
# decodes to the same value in both channels: there the rows are negatives or copies, bin by bin.
DECODED = [((2, 44100, 0.5, None), "dual_mono", "copies"), ((2, 44100, 1.0, None), "inverted", "negatives"),
           ((2, 44100, 0.5, None), "inverted", "negatives or copies"), ((6, 48000, 0.3, None), "all_same", "copies")]
DECODED_IDS = [f"{cid(c)}_{x}" for c, x, _ in DECODED]


@functools.lru_cache(maxsize=None)
def model_of(c):
    """-> (header packets, the model of tests/vorbis_model.py for them)"""
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(c[0], c[1], c[2])
    h = v.header_packets(setup)
    setup.close()
    return h, vm.Model(unpack_headers(*h), v.tables.pack("common.vpk")["FLOOR1_fromdB_LOOKUP"])


def model_spectra(oracle, c, image):
    """-> (headers, blocks, the model's result per packet): decoded once"""
    key = ("model", c, image)
    if key not in _cache:
        h, model = model_of(c)
        blks = blocks(oracle, c, image)
        _cache[key] = (h, blks, [model.decode(b["packet"]) for b in blks])
    return _cache[key]


def twins(c):
    """the channels that must decode alike: those that share a submap (floor and residue setup) with channel 0"""
    _, model = model_of(c)
    mux = model.s["maps"][0]["chmuxlist"]
    assert all(m["chmuxlist"] == mux for m in model.s["maps"])
    return [x for x in range(c[0]) if mux[x] == mux[0]]


def relation(a, b):
    """two float32 rows -> the number of bins that are non-zero exact negatives of one another (the sign bit alone
    differs), non-zero and bit-identical, and anything else but +0 in both"""
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    nz = (ua != 0) | (ub != 0)
    neg = nz & ((ua ^ np.uint32(0x80000000)) == ub)
    same = nz & (ua == ub)
    return int(neg.sum()), int(same.sum()), int((nz & ~neg & ~same).sum())


def check_relation(rows, chans, kind, what):
    """rows: per packet a [channels, n] float32 array; holds the rows of `chans` to `kind` and returns the counts"""
    neg = same = 0
    for k, r in enumerate(rows):
        for x in chans[1:]:
            a, b, other = relation(r[chans[0]], r[x])
            assert other == 0, (what, k, x)
            neg, same = neg + a, same + b
    if kind == "copies":
        assert neg == 0 and same >= 10000, (what, neg, same)
    elif kind == "negatives":
        assert same == 0 and neg >= 10000, (what, neg, same)
    else:
        assert neg >= 10000 and same >= 1000, (what, neg, same)
    return neg, same
