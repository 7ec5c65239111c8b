"""encode_ogg: whole files in batches.  File i's bytes are write_ogg of the packets the oracle makes of file i ALONE,
given to it as the reference application gives it (tests/encode_files_cases.py), with the file's own serial number —
whatever slot it ran in, however many slots there were and whatever else was in the list.  No tolerance."""
import struct

import pytest
import torch

from tests import encode_files_cases as fc

pytestmark = pytest.mark.gpu

STEREO_Q5 = (2, 44100, 0.5)
COMMENTS = ("TITLE=whole files",)


def serials(n):
    return [1000 + 77 * i for i in range(n)]


def wanted_files(v, oracle, cls, key, signals, serialnos, comments=COMMENTS):
    setup = v.Setup(*cls)
    seqs = fc.alone(oracle, cls, key, signals)
    out = [v.write_ogg(setup, [p for _, p in seq], [(m[5], m[4]) for m, _ in seq], sn, comments)
           for seq, sn in zip(seqs, serialnos)]
    setup.close()
    return out


def same_files(got, want, lengths):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert isinstance(a, bytes) and a == b, f"file {i} ({lengths[i]} samples) differs from the oracle's"


def page_serials(data):
    out, pos = [], 0
    while pos < len(data):
        assert data[pos:pos + 4] == b"OggS"
        out.append(struct.unpack_from("<I", data, pos + 14)[0])
        nseg = data[pos + 26]
        pos += 27 + nseg + sum(data[pos + 27:pos + 27 + nseg])
    return out


@pytest.mark.parametrize("how", [5, 1, 18, "reversed"])
def test_against_the_oracle(oracle, cuda, how):
    """18 files (every edge length, two with short blocks) over 5 slots, over 1, over one slot each, and the list
    reversed over 5: the same bytes per file"""
    import vorbis_aotuv_lancer_amd as v
    lengths, signals = fc.edge_files(oracle, STEREO_Q5)
    sn = serials(len(lengths))
    want = wanted_files(v, oracle, STEREO_Q5, "edge", signals, sn)
    if how == "reversed":
        got = v.encode_ogg(signals[::-1], 44100, 0.5, max_streams=5, serialnos=sn[::-1], comments=COMMENTS)[::-1]
    else:
        got = v.encode_ogg(signals, 44100, 0.5, max_streams=how, serialnos=sn, comments=COMMENTS)
    same_files(got, want, lengths)


@pytest.mark.parametrize("cls", [(1, 8000, 0.5), (6, 48000, 0.8), (2, 44100, None, 128000)],
                         ids=["1ch-8000-q0.5", "6ch-48000-q0.8", "2ch-44100-128k"])
def test_other_classes(oracle, cuda, cls):
    """{0, 1, a long block + 1, three long blocks + 1, 9000} samples over 3 slots (managed: the oracle's managed path,
    as tests/test_managed_oracle.py drives it)"""
    import vorbis_aotuv_lancer_amd as v
    lengths, signals = fc.small_files(oracle, cls)
    sn = serials(len(lengths))
    want = wanted_files(v, oracle, cls, "small", signals, sn)
    bitrate = cls[3] if len(cls) > 3 else None
    got = v.encode_ogg(signals, cls[1], cls[2], bitrate=bitrate, max_streams=3, serialnos=sn, comments=COMMENTS)
    same_files(got, want, lengths)


def test_round_trip_and_serial_numbers(oracle, cuda):
    """decode_ogg(encode_ogg(pcms)): exactly n_i samples per file at the input rate, none for the empty file; every
    page of file i carries serialnos[i]; numpy, host and device tensors are the same input"""
    import vorbis_aotuv_lancer_amd as v
    lengths, signals = fc.small_files(oracle, STEREO_Q5)
    sn = serials(len(lengths))
    files = v.encode_ogg(signals, 44100, max_streams=2, serialnos=sn)
    mixed = [torch.from_numpy(sig).to(cuda) if i % 3 == 0 else torch.from_numpy(sig) if i % 3 == 1 else sig
             for i, sig in enumerate(signals)]
    assert v.encode_ogg(mixed, 44100, max_streams=4, serialnos=sn) == files
    same_files(files, wanted_files(v, oracle, STEREO_Q5, "small", signals, sn, comments=()), lengths)
    for data, want_sn in zip(files, sn):
        pages = page_serials(data)
        assert len(pages) >= 3 and set(pages) == {want_sn}
        headers, packets, gps, eos = v.read_ogg(data)                 # CRCs, page order, one logical stream
        assert packets and eos[-1] and not any(eos[:-1])
    decoded = v.decode_ogg(files)
    assert len(decoded) == len(files)
    for (pcm, rate), L in zip(decoded, lengths):
        assert rate == 44100 and tuple(pcm.shape) == (2, L)
    # the default serial numbers are the files' indices
    plain = v.encode_ogg(signals[:3], 44100)
    assert [set(page_serials(d)) for d in plain] == [{0}, {1}, {2}]
