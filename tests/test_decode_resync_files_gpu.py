"""decode_ogg(resync=True) on the MI355X, on real encoded audio: undamaged files and a chain equal decode_ogg(chained=True)
bit for bit, and damaged ones (a lost page, a flipped byte, a tag in front) equal synthesis_runs over the packets and gap
marks the byte-serial model of the resync rules leaves (tests/ogg_resync_model.py), entry by entry and bit for bit."""
import numpy as np
import pytest

from tests import ogg_feed_resync_cases as RC
from tests import ogg_resync_file_cases as F
from tests.signals import burst_signal
from tests.test_decode_gaps_gpu import decode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def material(cuda):
    """two stereo 44.1 kHz q5 files of 2 s, and their chain"""
    import vorbis_aotuv_lancer_amd as v
    files = v.encode_ogg([burst_signal(2, 44100, 88200, seed=80 + i, period=5000) for i in range(2)], 44100, quality=0.5,
                         serialnos=[81, 82])
    for f in files:
        assert len(RC.audio_pages(f)) >= 5
    return v, files, files[0] + files[1]


def bits(pcm):
    return pcm.cpu().numpy().view(np.uint32)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert len(g) == len(w)
        for (a, ra), (b, rb) in zip(g, w):
            assert ra == rb and a.shape == b.shape and a.shape[1] > 0 and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("kw", ({}, {"device_demux": True}, {"device_demux": True, "one_decoder": True},
                                {"one_decoder": True, "halfrate": True}))
def test_undamaged_files_decode_as_chained(material, kw):
    v, files, chain = material
    given = files + [chain]
    want = v.decode_ogg(given, chained=True, **kw)
    assert [len(w) for w in want] == [1, 1, 2]
    same(v.decode_ogg(given, resync=True, **kw), want)


def damaged(files, chain):
    out = []
    for f in files + [chain]:
        ap = RC.audio_pages(f)
        k = ap[len(ap) // 2] if f is not chain else ap[-3]      # (the chain's: an audio page of its second link)
        out += [RC.without_pages(f, {k}), RC.flip(f, k, "body"), b"ID3" + bytes(range(125)) + f]
    return out + [b"ID3" + bytes(125), files[0][:20]]      # ... and two files that have no entry


def reference(v, blob):
    """-> per entry of the model (pcm [channels, n] as numpy uint32, samples per packet, the entry's packets)"""
    out = []
    for headers, pk in F.model_file(blob)[0]:
        ds = v.DecodeSetup(headers)
        dec = v.Decoder(ds, 1, 1024)
        pcm, n, samples, status = decode(dec, [0], [[p[:3] for p in pk]], [[p[3] for p in pk]])
        assert not status.cpu().numpy().any()
        out.append((bits(pcm[0, :, :int(n[0])]), samples.cpu().tolist(), pk))
        dec.close()
        ds.close()
    return out


@pytest.mark.parametrize("kw", ({}, {"device_demux": True}, {"device_demux": True, "one_decoder": True}))
def test_damaged_files_decode_as_the_models_packets(material, kw):
    v, files, chain = material
    given = damaged(files, chain)
    got = v.decode_ogg(given, resync=True, **kw)
    assert [len(g) for g in got] == [1, 1, 1] * 2 + [2, 2, 2] + [0, 0]
    for f, blob in enumerate(given):
        want = reference(v, blob)
        assert len(got[f]) == len(want), f
        for (pcm, rate), (ref, _, _) in zip(got[f], want):
            assert rate == 44100 and pcm.is_contiguous() and np.array_equal(bits(pcm), ref), f


def test_positions_in_front_of_the_hole_are_reached_exactly(material):
    """the samples returned through every packet that ends a page in front of the hole add up to that page's granule
    position"""
    v, files, _ = material
    for f in files:
        ap = RC.audio_pages(f)
        blob = RC.without_pages(f, {ap[len(ap) // 2]})
        (_, samples, pk), = reference(v, blob)
        hole = [k for k, p in enumerate(pk) if p[3]]
        assert len(hole) == 1
        at = np.cumsum(samples)
        front = [k for k in range(hole[0]) if pk[k][1] != -1]
        assert len(front) >= 2 and all(int(at[k]) == pk[k][1] for k in front)
        assert int(at[-1]) < pk[-1][1]                                    # ... and the hole's samples are missing behind it


def test_headers_no_setup_takes_raise(material):
    v, files, _ = material
    ps = [bytearray(p) for p in RC.pages(files[0])]
    from tests.ogg_pages import recrc
    ps[0][27 + ps[0][26] + 11] = 0                           # the identification header's channel count
    bad = RC.join([recrc(ps[0])] + ps[1:])
    for kw in ({}, {"device_demux": True}):
        with pytest.raises(v.VbmError, match="link 0"):
            v.decode_ogg([files[1], bad], resync=True, **kw)
    with pytest.raises(ValueError):
        v.decode_ogg(files, resync=True, multiplexed=True)
