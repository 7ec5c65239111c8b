"""The directed corpora (tests/reach_signals.py, tests/image_signals.py) at batch sizes where the launchers leave their
small-batch forms: the lane-per-channel-block floor fit instead of the cooperative one, coarse slices in offset-and-mix,
the floor render and the residue coder (csrc/batch.h, "kernel variants chosen by batch size").

K oracle-carved streams are replicated R times each: stream s of K * R carries signal s % K, so neighbouring lanes of a
wavefront hold different blocks, and every call holds all R copies of at least one signal.  Every size in here comes
from the product's own query (vorbis_aotuv_lancer_amd.batch_variants); no limit is written down twice.

What is compared, per call of Encoder.analysis_batch:
  * twins, on the device: for the packets, their lengths and every stage below, all rows of one signal equal that
    signal's first row, bit for bit (one reduction and one host sync per call);
  * the oracle, on the host: the at most K first rows, bit for bit.

Stages (VBR classes): poste, mdct_raw, logfft, logmdct, noise, tone, logmask, mdct, epeak, npeak, post_valid, nonzero,
residue (channels of a type-1 residue masked: encoded in place), and `post`.

`post`: the two captures are NOT taken at the same moment.  The oracle copies the posts as floor1_fit returns them
(values 0..1023, bit 15 = "this post is not worth coding").  The device's rows are read after the call, so they are as
floor1_encode left them: quantised by the floor's multiplier, and every post that is predicted exactly or was flagged
replaced by its prediction with bit 15 set, the flags of the neighbours of a coded post cleared.  That rewrite is a
function of the fitted posts and the floor's tables alone, so the oracle's capture is taken through it here
(encoded_posts: oracle/orc_floor1.c, the first loops of orc_floor1_encode, in numpy on the mode pack's tables) and the
result compared with the device's rows bit for bit: the first `posts` values of every row with post_valid set.  Rows
with post_valid == 0 and values past the floor's post count are written by nobody and are left out of both compares.

Managed classes: the device's logmask / epeak / npeak / residue rows are those of the last packetblob it worked on, the
oracle's capture is the middle blob's, so they are not compared; instead all fifteen packetblobs, the bitrate manager's
choice, and of the stages those that do not depend on the blob: poste, mdct_raw, logfft, logmdct, noise, tone, mdct,
and `post` (the middle blob's, as above)."""
import functools

import numpy as np

from tests import orc
from tests.encode_oracle import compare_blobs, lockstep, walk
from tests.image_signals import (all_same, alt_sign, delay1, dual_mono, front_same_rest_independent, hard_left,
                                 hard_left_dither, head, inverted, one_live, swap_mid_stream)
from tests.reach_signals import (click_trains, decaying_hits, edge_tones, faint_noise, gated_bands, nsamples,
                                 overdriven_noise, zero_tail)
from tests.signals import synth_signal

STAGES_F = ["poste", "mdct_raw", "logfft", "logmdct", "noise", "tone", "logmask", "mdct", "epeak", "npeak"]
STAGES_I = ["post_valid", "nonzero"]
MANAGED_F = ["poste", "mdct_raw", "logfft", "logmdct", "noise", "tone", "mdct"]
MINMAX = (144000, 128000, 112000)
SECONDS = 2.0


def synth(seed):
    return lambda ch, rate: synth_signal(ch, rate, nsamples(rate, SECONDS), seed=seed)


def case(name, ch, rate, q, bitrate, signals, seconds=SECONDS, res1_channels=(), sub_batches=1):
    return dict(name=name, ch=ch, rate=rate, q=q, bitrate=bitrate, signals=signals, seconds=seconds,
                res1_channels=res1_channels, sub_batches=sub_batches)


# the matrix: one GPU test per line (tests/test_large_batch_gpu.py), one set of witnesses per line (test_large_batch_cpu.py).
# The 5.1 cases are the first second of their signals and the managed min / max case the first 1.5 s: at 2 s they were the
# slowest tests of the file (the oracle's six channels and fifteen packetblobs included), as slow as or slower than
# tests/test_full_size_gpu.py::test_full_size_benchmarked_path; their witnesses hold on the shorter streams.  Cutting
# every case to 1 s loses witnesses (faint_noise's third level, zero_tail's tail, the packets cut under the maximum rate).
CASES = [
    case("2ch_44100_q0.5_reach", 2, 44100, 0.5, None, [("decaying_hits", decaying_hits), ("click_trains", click_trains),
                                                       ("faint_noise", faint_noise), ("inverted", inverted)]),
    case("2ch_44100_q0.5_edges", 2, 44100, 0.5, None, [("edge_tones", edge_tones), ("zero_tail", zero_tail),
                                                       ("gated_bands", gated_bands), ("dual_mono", dual_mono)]),
    case("1ch_44100_q0.1", 1, 44100, 0.1, None, [("decaying_hits", decaying_hits), ("click_trains", click_trains), ("synth", synth(831))]),
    case("2ch_44100_q-0.1", 2, 44100, -0.1, None, [("overdriven_noise", overdriven_noise), ("click_trains", click_trains),
                                                   ("decaying_hits", decaying_hits), ("hard_left", hard_left)]),
    case("6ch_48000_q0.3", 6, 48000, 0.3, None, [("decaying_hits", decaying_hits), ("alt_sign", alt_sign), ("one_live", one_live),
                                                 ("synth", synth(832))], seconds=1.0, res1_channels=(5,)),
    case("6ch_48000_q0.1", 6, 48000, 0.1, None, [("gated_bands", gated_bands),
                                                 ("front_same_rest_independent", front_same_rest_independent(0.1, None)),
                                                 ("synth", synth(833))], seconds=1.0, res1_channels=(5,)),
    case("2ch_22050_q0.5", 2, 22050, 0.5, None, [("click_trains", click_trains), ("decaying_hits", decaying_hits),
                                                 ("swap_mid_stream", swap_mid_stream)]),
    case("1ch_8000_q0.5", 1, 8000, 0.5, None, [("click_trains", click_trains), ("decaying_hits", decaying_hits), ("synth", synth(834))]),
    case("8ch_44100_q0.5", 8, 44100, 0.5, None, [("all_same", all_same), ("synth", synth(835))]),
    case("2ch_96000_q0.5", 2, 96000, 0.5, None, [("delay1", delay1), ("hard_left_dither", hard_left_dither), ("synth", synth(836))]),
    case("2ch_44100_b128000_max144000_min112000", 2, 44100, None, MINMAX,
         [("overdriven_noise", overdriven_noise), ("decaying_hits", decaying_hits), ("swap_mid_stream", swap_mid_stream)], seconds=1.5),
    case("2ch_44100_b256000", 2, 44100, None, 256000, [("faint_noise", faint_noise), ("decaying_hits", decaying_hits)]),
    case("2ch_44100_q0.5_two_sub_batches", 2, 44100, 0.5, None, [("decaying_hits", decaying_hits), ("click_trains", click_trains)],
         sub_batches=2),
]
CASE_IDS = [c["name"] for c in CASES]


def pack_of(c):
    import vorbis_aotuv_lancer_amd as v
    return v.tables.pack(orc.mode_pack_name(c["ch"], c["rate"], c["q"], c["bitrate"]))


def blocksizes(c):
    return tuple(int(x) for x in pack_of(c)["info/blocksizes"])


def block_types(c):
    """the block types the class has: one block size means no transition and no long blocks"""
    bs = blocksizes(c)
    return (0, 1) if bs[0] == bs[1] else (0, 1, 2, 3)


def streams_of(oracle, c):
    """the oracle's blocks of every signal of the case (1024 samples per write, end of stream declared): computed once"""
    out = []
    for name, make in c["signals"]:
        def pcm(make=make):
            x = head(make, c["seconds"])(c["ch"], c["rate"])
            assert x.shape[1] % 1024 == 0 and x.shape[1] <= 2 * c["rate"]
            return x
        out.append(walk(oracle, c["ch"], c["rate"], c["q"], c["bitrate"], pcm, key=("large_batch", name, c["seconds"])))
    assert 1 <= len(out) <= 4
    return out


# ---- sizes: everything from the product's query --------------------------------------------------------------------------
def slices_of(nsb, nsplit):
    """stream-blocks per slice of a batch under set_sub_batches(nsplit): whole 64-lane tiles, dealt as evenly as whole
    tiles allow (vbm_analysis_batch2); a slice is judged by its own size"""
    tiles = (nsb + 63) // 64
    nsplit = max(1, min(nsplit, tiles))
    out = []
    for part in range(nsplit):
        sb0, sb1 = tiles * part // nsplit * 64, min(tiles * (part + 1) // nsplit * 64, nsb)
        if sb1 > sb0:
            out.append(sb1 - sb0)
    return out


def call_mask(block_mode, n, ch, nsb, nsplit=1):
    """the variants one call takes: bits 0..3 are those every slice of it takes, bit 4 is decided on the whole batch"""
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd.encoder import LARGE_BATCH_BITS, MIX_MAKES_FIT_WORDS
    mask = LARGE_BATCH_BITS
    for part in slices_of(nsb, nsplit):
        mask &= v.batch_variants(block_mode, n, ch, part)
    return mask | (v.batch_variants(block_mode, n, ch, nsb) & MIX_MAKES_FIT_WORDS)


def wanted_bits(block_mode):
    """every large form the block type can take: impulse blocks are not sliced in offset-and-mix"""
    from vorbis_aotuv_lancer_amd.encoder import COARSE_BIN_SLICES, LARGE_BATCH_BITS
    return LARGE_BATCH_BITS & ~COARSE_BIN_SLICES if block_mode == 0 else LARGE_BATCH_BITS


@functools.lru_cache(maxsize=None)
def pick_R(ch, sizes=(256, 2048), nsplit=1, most_signals=4):
    """The smallest R for which a call of nsb = R stream-blocks (and, sliced, of R .. most_signals * R) takes every large
    form in every block type of both block sizes, then raised until neither R nor R * ch is a multiple of 64: the last
    wavefront of the lean floor fit and the last tile are partial."""
    def large(R):
        return all(call_mask(m, N // 2, ch, R * j, nsplit) & wanted_bits(m) == wanted_bits(m)
                   for N in sizes for m in range(4) for j in (range(1, most_signals + 1) if nsplit > 1 else (1,)))
    lo, hi = 0, 1
    while not large(hi):        # (the forms are monotone in the size: small below a limit, large above it)
        lo, hi = hi, hi * 2
        assert hi < 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if large(mid) else (mid, hi)
    R = hi
    while R % 64 == 0 or (R * ch) % 64 == 0 or not large(R):
        R += 1
    return R


def R_of(c):
    return pick_R(c["ch"], blocksizes(c), c["sub_batches"], len(c["signals"]))


def replicated_schedule(streams, R):
    """lockstep(streams, R) of tests/encode_oracle.py without the blocks: [(k, block_mode, signals present, stream ids)]"""
    return [call[:4] for call in lockstep(streams, R)]


def schedule_masks(c, streams, R):
    """per block type, the set of masks its calls take"""
    seen = {}
    for k, mode, present, ids in replicated_schedule(streams, R):
        N = streams[present[0]][k]["N"]
        seen.setdefault(mode, set()).add(call_mask(mode, N // 2, c["ch"], len(ids), c["sub_batches"]))
    return seen


# ---- `post` as floor1_encode leaves it ------------------------------------------------------------------------------------
def floors_of(c, W):
    """per channel of block size W: (posts, multiplier, post positions, low neighbours, high neighbours)"""
    d = pack_of(c)
    nmaps = int(d["info/counts"][1])
    mp = int(d[f"mode/{W}"][3]) if W < nmaps else 0
    out = []
    for ch in range(c["ch"]):
        f = int(d[f"map/{mp}/floorsubmap"][int(d[f"map/{mp}/chmuxlist"][ch])])
        posts = 2 + sum(int(d[f"floor/{f}/class_dim"][int(d[f"floor/{f}/partitionclass"][i])]) for i in range(int(d[f"floor/{f}/partitions"][0])))
        X = [int(x) for x in d[f"floor/{f}/postlist"][:posts]]
        lo = [max((j for j in range(i) if X[j] < X[i]), key=lambda j: X[j]) for i in range(2, posts)]
        hi = [min((j for j in range(i) if X[j] > X[i]), key=lambda j: X[j]) for i in range(2, posts)]
        out.append((posts, int(d[f"floor/{f}/mult"][0]), X, lo, hi))
    return out


def encoded_posts(post, floor):
    """one channel's fitted posts -> the same after the quantising and predicting loops of floor1_encode"""
    posts, mult, X, lo, hi = floor
    p = [int(x) for x in post[:posts]]
    for i in range(posts):
        val = p[i] & 0x7fff
        val = {1: val >> 2, 2: val >> 3, 3: val // 12, 4: val >> 4}[mult]
        p[i] = val | (p[i] & 0x8000)
    for i in range(2, posts):
        ln, hn = lo[i - 2], hi[i - 2]
        y0, y1 = p[ln] & 0x7fff, p[hn] & 0x7fff
        off = abs(y1 - y0) * (X[i] - X[ln]) // (X[hn] - X[ln])
        predicted = y0 - off if y1 < y0 else y0 + off
        if (p[i] & 0x8000) or predicted == p[i]:
            p[i] = predicted | 0x8000
        else:
            p[ln] &= 0x7fff
            p[hn] &= 0x7fff
    return np.array(p, np.int32)


def run_case(oracle, cuda, c):
    """-> dict(blocks = lead blocks compared with the oracle, calls, masks = {block type: set of masks}, rows = rows held
    to their twins, R): run_lockstep of tests/encode_calls.py with R replicas; `post`, and in managed classes the
    packetblobs, the choice and `nonzero` (twins only: the device's is the last packetblob's), are added per call here"""
    import torch
    import vorbis_aotuv_lancer_amd as v
    from tests.encode_calls import packet_words, run_lockstep
    ch, managed = c["ch"], c["bitrate"] is not None
    streams = streams_of(oracle, c)
    R = R_of(c)
    setup = v.Setup(ch, c["rate"], bitrate=c["bitrate"]) if managed else v.Setup(ch, c["rate"], c["q"])
    enc = v.Encoder(setup, len(streams) * R)
    if c["sub_batches"] > 1:
        enc.set_sub_batches(c["sub_batches"])
    floors = [floors_of(c, W) for W in (0, 1)]
    masks = {}

    def more(call):
        Km, nsb, mode = len(call.present), len(call.ids), call.mode
        masks.setdefault(mode, set()).add(call_mask(mode, call.blks[0]["N"] // 2, ch, nsb, c["sub_batches"]))
        post = enc.fetch("post")
        posts = torch.tensor([floors[mode >> 1][x][0] for x in range(ch)], device=cuda).repeat(nsb)
        ok = (call.got["post_valid"] != 0)[:, None] & (torch.arange(post.shape[1], device=cuda)[None, :] < posts[:, None])
        call.held.append(("post", post, ok, ch))
        lead = post[:Km * ch].cpu().numpy()
        for i, b in enumerate(call.blks):
            for x in range(ch):
                if b["post_valid"][x]:
                    fl = floors[mode >> 1][x]
                    want = encoded_posts(b["post"][x], fl)
                    assert np.array_equal(lead[i * ch + x, :fl[0]], want), (call.label, "post", i, x, lead[i * ch + x, :fl[0]], want)
        if managed:
            choice = enc.fetch("choice")
            blobs = [enc.fetch_blob(kb) for kb in range(15)]
            call.held += [("nonzero", enc.fetch("nonzero"), None, ch), ("choice", choice, None, 1)]
            for kb, (bp, bn) in enumerate(blobs):
                call.held += [(f"blob {kb} lengths", bn, None, 1), (f"blob {kb}", bp, packet_words(bp, bn), 1)]
            compare_blobs([(bp[:Km].cpu().numpy(), bn[:Km].cpu().numpy()) for bp, bn in blobs], choice[:Km].cpu().numpy(),
                          call.blks, call.label, cut=True)

    stat = run_lockstep(enc, cuda, streams, ch, MANAGED_F if managed else STAGES_F,
                        STAGES_I[:1] if managed else STAGES_I + ["residue"], c["res1_channels"], R=R, on_call=more, label=c["name"])
    enc.close()
    setup.close()
    return dict(stat, masks=masks, R=R)

