"""The device against the oracle on the correlated-channel corpus (tests/image_signals.py): dual mono, inverted pairs,
near-mono, a gain-only pan, a dead channel — inputs that put couple/quantise on its exact ties (A = +-B in lossless
coupling, a = -b in the point-coupling hypot, an M6 residue_def of 0, equal nepeak values handed over, angle vectors of
0 and of -2 |magnitude|).  tests/test_images_cpu.py shows on the oracle alone that the corpus gets there.  Everything
here is bit for bit, with no tolerance anywhere.

  * Stage by stage (run_stages of tests/encode_calls.py: vbm_analysis_batch on oracle-carved blocks), image streams
    and synth_signal streams in one batch, so partitions on a tie share a 64-lane tile with partitions that are not.
  * From PCM through the stream front end, every class of the corpus, the managed ones included.
  * Managed, blob by blob: all fifteen packetblobs, the choice and the delivered packet of every block.
  * The decoder on the oracle's packets: the spectrum is the model's (tests/vorbis_model.py), and the PCM channels are
    copies or exact negatives of one another where the spectra are.

Which couple kernel a block lands on (capi_encoder.cpp, configure): long blocks with 32-bin partitions take
k_couple_fast, mode 2 for stereo and mode 1 for the uncoupled setups; blocks with 8-bin partitions (every short block,
and both block sizes of 2ch 22050) take k_couple_m6stats + k_couple_quantize sliced over partitions; coupled 5.1, whose
channel 0 serves in three steps, takes k_couple_quantize as one serial chunk in both block sizes.  Managed mode runs
the blob loop on top of each."""
import pytest

from tests.encode_calls import frontend_vs_oracle, managed_blobs, run_stages
from tests.image_cases import DECODED, check_relation, cid, model_spectra, twins
from tests.image_signals import MINMAX, SECONDS, classes, images_of, seconds_of
from tests.reach_signals import nsamples
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu


def makers_of(ch, rate, q=None, bitrate=None, only=None, nsynth=2, seed=840):
    """(name, make) of the class's images with `nsynth` synth_signal streams among them; the name is the key of the oracle walk's cache"""
    out, secs = [], seconds_of(ch, rate, q, bitrate)
    for e in images_of(ch, rate, q, bitrate):
        if only is None or any(e["name"].startswith(x + "_%dch" % ch) for x in only):
            out.append((e["name"], lambda e=e: e["make"](e["ch"], e["rate"])))
    assert len(out) == (len(images_of(ch, rate, q, bitrate)) if only is None else len(only))
    for k in range(nsynth):
        name = f"synth_beside_images_{seed + k}"
        out.insert(min(2 * k + 1, len(out)), (name, lambda k=k: synth_signal(ch, rate, nsamples(rate, secs), seed=seed + k)))
    return out


STAGE_CLASSES = [(2, 44100, 0.5, ()), (2, 44100, -0.1, ()), (2, 44100, 1.0, ()), (2, 22050, 0.5, ()), (6, 48000, 0.3, (5,))]


@pytest.mark.parametrize("ch,rate,q,res1_channels", STAGE_CLASSES, ids=[cid(c[:3] + (None,)) for c in STAGE_CLASSES])
def test_stages(oracle, cuda, ch, rate, q, res1_channels):
    """mdct_raw, logfft, logmdct, noise, tone, logmask, mdct, epeak, npeak, post_valid, nonzero, residue and the packet
    of every block of every image of the class (and poste, which is -1 throughout)"""
    makers = makers_of(ch, rate, q)
    assert len(makers) >= 6
    c = run_stages(oracle, cuda, ch, rate, q, makers, res1_channels=res1_channels)
    assert c["blocks"] >= 40 * len(makers) and c["poste"] == 0


@pytest.mark.parametrize("c", classes(), ids=cid)
def test_from_pcm(oracle, cuda, c):
    """the class's images and synth_signal streams, interleaved, through the stream front end: block headers (lW, W,
    nW, mode, e_o_s, granule position, packet number) and packets are the oracle's"""
    ch, rate, q, bitrate = c
    images = images_of(*c)
    sigs = [make() for _, make in makers_of(ch, rate, q, bitrate, nsynth=max(2, 6 - len(images)), seed=850)]
    assert len(sigs) >= 6 and len({s.shape for s in sigs}) == 1
    frontend_vs_oracle(oracle, cuda, ch, rate, q, NS=len(sigs), seconds=seconds_of(*c), bitrate=bitrate, sigs=sigs,
                       need_modes=(0, 1) if rate < 16000 else (0, 1, 2, 3))


@pytest.mark.parametrize("bitrate", [128000, MINMAX], ids=["b128000", "b128000_minmax"])
def test_managed_blobs_block_by_block(oracle, cuda, bitrate):
    """2ch 44100 managed on dual mono (the manager chooses blobs 7 .. 12), inverted (4 .. 7), near-mono at -80 dB and
    the stream that swaps from the one to the other half way: in every point-coupled partition of every blob the angle
    channel's nepeak is handed to the magnitude channel with both values equal"""
    makers = makers_of(2, 44100, None, bitrate, only=["dual_mono", "inverted", "near_mono_80", "swap_mid_stream"], nsynth=1,
                       seed=860)
    nblocks, nposte, ncut = managed_blobs(oracle, cuda, bitrate, makers)
    assert nblocks > 400 and nposte == 0


DECODE_SETUPS = []
for _c, _image, _kind in DECODED:
    if _c not in DECODE_SETUPS:
        DECODE_SETUPS.append(_c)


@pytest.mark.parametrize("c", DECODE_SETUPS, ids=cid)
def test_decoder_on_copies_and_negatives(oracle, cuda, c):
    """The oracle's packets of dual mono and the inverted pair at q0.5 (where some bins are point-coupled), of the
    inverted pair at q1.0 (where every bin stays lossless) and of 5.1 with one signal in every channel, decoded with
    synthesis_runs: the streams of a setup are the runs of one call.  Unpack and spectrum are the model's for every
    packet.  The PCM channels are bit-identical where the spectrum rows are, and exact negatives where those are: the
    inverse MDCT, the window and the overlap-add are sums and products, which round alike for x and -x.  (Inverted at
    q0.5 decodes to a mix of negated and copied bins, so its PCM has no such property; its spectrum is compared.)"""
    import vorbis_aotuv_lancer_amd as v
    from tests.decode_calls import against_model, runs_call
    streams = [(image, kind) for c2, image, kind in DECODED if c2 == c]
    decoded = [model_spectra(oracle, c, image) for image, _ in streams]
    runs = [[(b["packet"], b["granulepos"], b["eos"]) for b in blks] for _, blks, _ in decoded]
    ds = v.DecodeSetup(decoded[0][0])
    dec = v.Decoder(ds, len(runs), sum(len(r) for r in runs))
    pcm, run_samples, samples, status = runs_call(dec, list(range(len(runs))), runs, cuda)
    samples, status = samples.cpu().numpy(), status.cpu().numpy()
    assert not status.any()
    got = against_model(dec, [r for _, _, results in decoded for r in results], status, samples, cid(c))
    pcm, run_samples = pcm.cpu().numpy(), run_samples.cpu().numpy()
    chans = twins(c)
    at = 0
    for r, (image, kind) in enumerate(streams):
        rows = got["spectrum"][at:at + len(runs[r])]
        at += len(runs[r])
        check_relation(rows, chans, kind, f"{cid(c)} {image} spectrum")
        assert run_samples[r] == nsamples(c[1], SECONDS)
        if kind != "negatives or copies":
            neg, same = check_relation([pcm[r][:, :run_samples[r]]], chans, kind, f"{cid(c)} {image} pcm")
            print(f"{cid(c)} {image}: {run_samples[r]} samples per channel, {neg} exact negatives, {same} bit-identical")
    dec.close()
    ds.close()
