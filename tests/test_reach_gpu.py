"""The device against the oracle on the reach corpus (tests/reach_signals.py): PCM that takes the oracle branches the
synth_signal / burst_signal family never takes ("Oracle branches: which ones the tests reach"), above
all aoTuV's M2 post-echo reduction: k_prologue's detector, the `s_poste` arm of k_noisemask and the npeak = -1 it
hands to offset-and-mix and to couple/quantise.

Stage by stage (run_stages / managed_blobs of tests/encode_calls.py: vbm_analysis_batch on oracle-carved blocks, like
tests/test_pipeline_gpu.py, shared with tests/test_images_gpu.py): every stage that file
compares, and for every block three it does not: `poste`, `epeak` and `npeak`, bit for bit.

  * `npeak` is compared as couple/quantise leaves it, which is where the oracle captures it: both sides rewrite the
    magnitude channel's entry where they point-couple.  The device writes every one of its n / partition rows in
    k_noisemask, so no row is masked.  It is not compared in the managed case: there the fifteen packetblobs hand the
    rows on to one another and the oracle's capture is taken after blob 7, the device's rows after blob 14; the blobs
    themselves are compared instead, every one of them.
  * `residue` of a channel that goes through a type-1 residue is masked as in test_pipeline_gpu (encoded in place).

From PCM (the stream front end, like tests/test_vq_edges_gpu.py): block headers and packets, byte for byte, in batches
that put reach streams and synth_signal streams side by side in one 64-lane tile, so that blocks with poste > 0 sit next
to blocks without."""
import pytest

from tests.encode_calls import frontend_vs_oracle, managed_blobs, run_stages
from tests.reach_signals import REACH, click_trains, decaying_hits, faint_noise, gated_bands, nsamples, overdriven_noise
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu

SECONDS = 2.0


def synth(ch, rate, seed):
    return synth_signal(ch, rate, nsamples(rate, SECONDS), seed=seed)


def test_stages_stereo_q5(oracle, cuda):
    c = run_stages(oracle, cuda, 2, 44100, 0.5, [("decaying_hits", lambda: decaying_hits(2, 44100)), ("synth", lambda: synth(2, 44100, 801)),
                                                 ("click_trains", lambda: click_trains(2, 44100))])
    assert c["poste"] >= 3 and c["minus1"] > 0 and c["mixed"] > 0


def test_stages_mono_q1(oracle, cuda):
    c = run_stages(oracle, cuda, 1, 44100, 0.1, [("decaying_hits", lambda: decaying_hits(1, 44100)), ("synth", lambda: synth(1, 44100, 802))])
    assert c["poste"] >= 3 and c["minus1"] > 0


def test_stages_coupled_51_q3(oracle, cuda):
    c = run_stages(oracle, cuda, 6, 48000, 0.3, [("decaying_hits", lambda: decaying_hits(6, 48000)), ("synth", lambda: synth(6, 48000, 803))],
                   res1_channels=(5,))
    assert c["poste"] >= 3 and c["minus1"] > 0 and c["mixed"] > 0


def test_stages_short_blocks_of_512_at_44k(oracle, cuda):
    """2ch 44100 q-0.1 (512 / 4096): set_m3p's n = 256 case with runs of impulse blocks and impulses after padding,
    and the post-echo reduction in blocks of 4096"""
    c = run_stages(oracle, cuda, 2, 44100, -0.1, [("click_trains", lambda: click_trains(2, 44100)), ("decaying_hits", lambda: decaying_hits(2, 44100)),
                                                  ("synth", lambda: synth(2, 44100, 804))])
    assert c["poste"] >= 3


def test_stages_blocks_of_512_at_8k(oracle, cuda):
    c = run_stages(oracle, cuda, 1, 8000, 0.5, [("click_trains", lambda: click_trains(1, 8000)), ("synth", lambda: synth(1, 8000, 805))])
    assert c["poste"] == 0          # one block size: no transition blocks, the detector never passes its mode test


# ---- from PCM ---------------------------------------------------------------------------------------------------------
def mixed(ch, rate, reach):
    """the reach streams with synth_signal streams between them: 6 to 8 streams, at least two of them synth_signal"""
    assert len(reach) <= 6
    nsynth = max(6 - len(reach), 2)
    out = []
    for k, x in enumerate(reach):
        out.append(x)
        if k < nsynth:
            out.append(synth(ch, rate, 820 + k))
    out += [synth(ch, rate, 820 + k) for k in range(len(reach), nsynth)]
    return out


def by_class(ch, rate, q=None, bitrate=None):
    return [e["make"](ch, rate) for e in REACH if (e["ch"], e["rate"], e["q"], e["bitrate"]) == (ch, rate, q, bitrate)]


FROM_PCM = [
    # (channels, rate, q, bitrate, further streams of the class beside REACH's own)
    (2, 44100, 0.5, None, lambda: []),
    (1, 44100, 0.1, None, lambda: [decaying_hits(1, 44100, seed=15), click_trains(1, 44100)]),
    (6, 48000, 0.3, None, lambda: [decaying_hits(6, 48000, seed=16, solo=1)]),
    (6, 48000, 0.1, None, lambda: [gated_bands(6, 48000, seed=18), decaying_hits(6, 48000)]),
    (2, 44100, -0.1, None, lambda: []),
    (1, 8000, 0.5, None, lambda: [click_trains(1, 8000, seed=17), decaying_hits(1, 8000)]),
    (2, 22050, 0.5, None, lambda: [click_trains(2, 22050), decaying_hits(2, 22050, seed=19)]),
    (2, 44100, None, 128000, lambda: [decaying_hits(2, 44100, seed=20), click_trains(2, 44100)]),
    (2, 44100, None, 256000, lambda: [faint_noise(2, 44100, seed=21), decaying_hits(2, 44100)]),
    (2, 44100, None, (144000, 128000, 112000), lambda: [overdriven_noise(2, 44100, seed=22), decaying_hits(2, 44100)]),
]


def test_from_pcm_covers_the_corpus():
    have = {(c[0], c[1], c[2], c[3]) for c in FROM_PCM}
    assert {(e["ch"], e["rate"], e["q"], e["bitrate"]) for e in REACH} == have


def class_id(c):
    ch, rate, q, bitrate = c[:4]
    if bitrate is None:
        return f"{ch}ch_{rate}_q{q:g}"
    return f"{ch}ch_{rate}_b{bitrate}" if isinstance(bitrate, int) else "%dch_%d_b%d_max%d_min%d" % (ch, rate, bitrate[1], bitrate[0], bitrate[2])


@pytest.mark.parametrize("ch,rate,q,bitrate,more", FROM_PCM, ids=[class_id(c) for c in FROM_PCM])
def test_from_pcm(oracle, cuda, ch, rate, q, bitrate, more):
    """every reach signal of the class plus synth_signal streams, interleaved, through the stream front end: block
    headers (lW, W, nW, mode, e_o_s, granule position, packet number) and packets are the oracle's"""
    sigs = mixed(ch, rate, by_class(ch, rate, q, bitrate) + more())
    assert len(sigs) >= 6 and len({s.shape for s in sigs}) == 1
    frontend_vs_oracle(oracle, cuda, ch, rate, q, NS=len(sigs), seconds=SECONDS, bitrate=bitrate, sigs=sigs,
                       need_modes=(0, 1) if rate < 16000 else (0, 1, 2, 3))


BLOB_CASES = [
    (128000, [("decaying_hits", lambda: decaying_hits(2, 44100)), ("synth", lambda: synth(2, 44100, 806)),
              ("decaying_hits_20", lambda: decaying_hits(2, 44100, seed=20))], 3),
    (256000, [("faint_noise", lambda: faint_noise(2, 44100)), ("synth", lambda: synth(2, 44100, 807))], 0),
    ((144000, 128000, 112000), [("overdriven_noise", lambda: overdriven_noise(2, 44100)), ("synth", lambda: synth(2, 44100, 808))], 0),
]



@pytest.mark.parametrize("bitrate,makers,min_poste", BLOB_CASES, ids=["b128000_hits", "b256000_faint", "b128000_minmax_overdriven"])
def test_managed_blobs_block_by_block(oracle, cuda, bitrate, makers, min_poste):
    """2ch 44100 managed: all fifteen packetblobs, the bitrate manager's choice and the packets of every block.
    Decaying hits at b128000: the blobs' coupling passes hand the npeak rows on to one another, and here rows of -1 from
    the post-echo arm enter that chain.  Faint noise at b256000: blocks with a floor at the middle rate and none at a
    neighbouring one, so interpolated fits come out empty.  Overdriven noise under a maximum rate: the manager runs out
    of smaller blobs and cuts the packet."""
    nblocks, nposte, ncut = managed_blobs(oracle, cuda, bitrate, makers)
    assert nposte >= min_poste
    assert (ncut > 0) == isinstance(bitrate, tuple)
