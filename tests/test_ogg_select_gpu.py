"""The Vorbis stream of multiplexed Ogg files, picked on the device (vbm_ogg_select): equal to its host twin byte for byte
on the corpora of the CPU file, at every alignment of source and destination and around the copy kernel's chunk edges;
demux_ogg_device, decode_ogg and OggIndex with multiplexed=True against the Vorbis-only files; the defaults unchanged;
two selectors on two streams."""
import numpy as np
import pytest
import torch

from tests import ogg_demux_batch as B
from tests import ogg_select_cases as S
from tests.ogg_select_cases import ECAP, EINVAL, EOGG
from tests.signals import synth_signal
from tests.ogg_pages import split_pages

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", S.GROUPS)
def test_device_equals_host_twin(cuda, group):
    """each corpus group as one batch: output, offsets and info, into a buffer of exactly the kept total with a guard
    behind it, and once more with the input's size as the capacity"""
    blobs = S.group(group)
    d = S.check_twin(blobs)
    S.check_twin(blobs, out_cap=sum(len(b) for b in blobs))
    want_out, want_off, want_info = S.expected(blobs)           # the twin is pinned to the model in the CPU file
    assert d.out.tobytes() == want_out and np.array_equal(d.out_offsets, want_off) and S.same_info(d.info, want_info)


def test_alignment_corpus_covers_every_pair_and_length():
    pairs, lengths = S.alignment_coverage(S.alignment_files())
    assert not {(a, b) for a in range(16) for b in range(16)} - pairs
    assert not set(range(27, 27 + 65)) - lengths


@pytest.mark.parametrize("first", range(16))
def test_every_alignment_of_source_and_destination(cuda, first):
    S.check_twin(S.alignment_files(), first)


@pytest.mark.parametrize("first", [0, 1, 15])
def test_chunk_edges_at_other_alignments(cuda, first):
    S.check_twin(S.chunk_files(), first)


def test_capacity_one_short_writes_nothing(cuda):
    blobs = [m for _, m, _ in S.singles()]
    data, offsets = B.pack(blobs)
    want_out, want_off, want_info = S.expected(blobs)
    s = S.Select("device", len(blobs), len(data))
    try:
        r = s.select(data, offsets, len(want_out) - 1)
        assert r.status == ECAP and not r.touched and r.guard_ok
        assert np.array_equal(r.out_offsets, want_off) and S.same_info(r.info, want_info)
        r = s.select(data, offsets, len(want_out))
        assert r.status == 0 and r.out.tobytes() == want_out and r.guard_ok
    finally:
        s.close()


def test_device_call_refuses_a_host_object_and_bad_arguments(cuda):
    blob = S.case1()["skeleton first"][0]
    data, off = B.pack([blob])
    d = torch.from_numpy(data.copy()).cuda()
    out = torch.zeros(len(blob), dtype=torch.uint8, device="cuda")
    meta = torch.zeros(16, dtype=torch.int64, device="cuda")
    host, dev = S.Select("host", 1, len(blob)), S.Select("device", 1, len(blob))
    try:
        ok = (1, d.data_ptr(), off.ctypes.data, out.data_ptr(), len(blob), meta.data_ptr(), meta.data_ptr() + 16)
        host.impl, dev.impl = "device", "host"               # each call form with the other kind of object
        assert host.select_raw(*ok) == EINVAL and dev.select_raw(*ok) == EINVAL
        host.impl, dev.impl = "host", "device"
        assert dev.select_raw(2, *ok[1:]) == EINVAL and dev.select_raw(*ok[:4], -1, *ok[5:]) == EINVAL
        for k in (1, 2, 3, 5, 6):
            assert dev.select_raw(*ok[:k], None, *ok[k + 1:]) == EINVAL
        assert dev.select_raw(*ok[:3], d.data_ptr() + 100, *ok[4:]) == EINVAL      # in place
        assert dev.select_raw(*ok) == 0 and dev.status() == 0
        assert meta.cpu().numpy()[:2].tolist() == [0, len(S.model(blob)[0])]
    finally:
        host.impl, dev.impl = "host", "device"
        host.close()
        dev.close()


def _same_batch(got, want):
    assert got.status == want.status and got.headers == want.headers
    assert np.array_equal(got.file_links, want.file_links) and got.names == want.names
    assert got.info.tobytes() == want.info.tobytes()
    for name in ("payload", "offsets", "granulepos", "eos"):
        assert getattr(got, name).is_cuda and torch.equal(getattr(got, name), getattr(want, name)), name


def test_demux_ogg_device_multiplexed(cuda):
    import vorbis_aotuv_lancer_amd as v
    one = [s for s in S.singles() if s[0] not in S.case5()]
    got = v.demux_ogg_device([m for _, m, _ in one], multiplexed=True)
    want = v.demux_ogg_device([w for _, _, w in one])
    assert not any(got.status) and want.select_info is None
    _same_batch(got, want)
    twin = v.demux_ogg_device([m for _, m, _ in one], host=True, multiplexed=True)
    assert got.select_info.tobytes() == twin.select_info.tobytes()
    c5 = list(S.case5().values())
    got = v.demux_ogg_device([m for m, _ in c5], chained=True, multiplexed=True)
    want = v.demux_ogg_device([w for _, w in c5], chained=True)
    assert not any(got.status) and got.file_links.tolist() == [0, 2, 5, 7]
    _same_batch(got, want)


def test_defaults_are_unchanged(cuda):
    """without the keyword: VBM_EOGG per entry, and with chained=True the two-link shape of a multiplexed start"""
    import vorbis_aotuv_lancer_amd as v
    files = [m for _, m, _ in S.singles()]
    b = v.demux_ogg_device(files)
    assert b.status == [EOGG] * len(files) and b.select_info is None
    b = v.demux_ogg_device([S.case1()["skeleton first"][0]], chained=True)
    assert b.status == [EOGG, EOGG] and b.file_links.tolist() == [0, 2]
    b, h = v.demux_ogg_device(files, chained=True), v.demux_ogg_device(files, host=True, chained=True)
    assert b.status == h.status and np.array_equal(b.file_links, h.file_links) and EOGG in b.status
    with pytest.raises(v.VbmError, match="file 0"):
        v.decode_ogg(files[:1], device_demux=True)


# ---- decoding: real audio between the foreign pages ---------------------------------------------------------------------

def _p(blob):
    return [bytes(p) for p in split_pages(blob)]


@pytest.fixture(scope="module")
def encoded(cuda):
    """short encoded files in two classes, each muxed with foreign streams the ways of cases 1 to 5, and the Vorbis-only
    files decoded"""
    import vorbis_aotuv_lancer_amd as v
    st = v.encode_ogg([synth_signal(2, 44100, n, seed=70 + i) for i, n in enumerate((15000, 9000, 13001))], 44100,
                      quality=0.5, serialnos=[31, 32, 33])
    mono = v.encode_ogg([synth_signal(1, 8000, 3000, seed=80)], 8000, quality=0.5, serialnos=[41])[0]
    sk = S.foreign("skeleton", 71, 1, sizes=(80, 600, 80))
    th = S.foreign("theora", 72, 2, sizes=(150000, 30, 66000), max_segs=255)
    plain = [st[0], st[1], mono, st[2]]
    muxed = [S._cat([sk[0], _p(st[0])[0]] + sk[1:] + _p(st[0])[1:]),                      # Skeleton first
             S._cat(S.interleave([th, _p(st[1])], 3)),                                    # video-like
             S._cat(S.interleave([_p(mono), S.foreign("theora", 73, 4)], 5)),             # Vorbis head first
             S._cat(S.interleave([S.foreign("opus", 74, 6), _p(st[2]), _p(mono)], 7))]    # two Vorbis streams
    chains = [[st[0], mono], [st[1], st[2]]]
    none = S.interleave([S.foreign("theora", 82, 20), S.foreign("opus", 83, 21)], 22)
    muxed_chains = [muxed[0] + muxed[2], S._cat(S.interleave([_p(st[1]), S.foreign("opus", 31, 8)], 9) + none) + muxed[3]]
    for m, w in zip(muxed + muxed_chains, plain + [b"".join(c) for c in chains]):
        assert S.model(m)[0] == w
    ref = {half: v.decode_ogg(plain, halfrate=half) for half in (False, True)}
    return plain, muxed, chains, muxed_chains, ref


def _equal(got, ref):
    assert len(got) == len(ref)
    for k, ((pcm, rate), (want, want_rate)) in enumerate(zip(got, ref)):
        assert rate == want_rate and pcm.shape == want.shape and pcm.shape[1] > 0 and torch.equal(pcm, want), k


@pytest.mark.parametrize("device_demux", [True, False])
def test_decode_ogg_multiplexed(cuda, encoded, device_demux):
    import vorbis_aotuv_lancer_amd as v
    plain, muxed, _, _, ref = encoded
    _equal(v.decode_ogg(muxed, multiplexed=True, device_demux=device_demux), ref[False])
    _equal(v.decode_ogg(plain, multiplexed=True, device_demux=device_demux), ref[False])      # plain files: identity
    if device_demux:
        _equal(v.decode_ogg(muxed[:2], multiplexed=True, device_demux=True, halfrate=True), ref[True][:2])


@pytest.mark.parametrize("device_demux", [True, False])
def test_decode_ogg_multiplexed_chained(cuda, encoded, device_demux):
    import vorbis_aotuv_lancer_amd as v
    _, _, chains, muxed_chains, _ = encoded
    got = v.decode_ogg(muxed_chains, multiplexed=True, chained=True, device_demux=device_demux)
    want = v.decode_ogg([b"".join(c) for c in chains], chained=True)
    assert [len(g) for g in got] == [2, 2]
    for g, w in zip(got, want):
        _equal(g, w)


@pytest.mark.parametrize("device_demux", [True, False])
def test_decode_ogg_names_the_file_without_a_vorbis_stream(cuda, encoded, device_demux):
    import vorbis_aotuv_lancer_amd as v
    _, muxed, _, _, _ = encoded
    for chained in (False, True):
        with pytest.raises(v.VbmError, match="file 1.*no Vorbis stream"):
            v.decode_ogg([muxed[0], S.case6()["opus-like"]], multiplexed=True, device_demux=device_demux, chained=chained)


@pytest.mark.parametrize("device_demux", [True, False])
def test_ogg_index_multiplexed(cuda, encoded, device_demux):
    """one header class: the three stereo files"""
    import vorbis_aotuv_lancer_amd as v
    plain, muxed, _, _, _ = encoded
    ids = [0, 1, 3]
    want = v.OggIndex([plain[i] for i in ids])
    got = v.OggIndex([muxed[i] for i in ids], device_demux=device_demux, multiplexed=True)
    try:
        assert np.array_equal(got.total_samples, want.total_samples) and (got.total_samples > 0).all()
        files = np.repeat(np.arange(3), 3)
        starts = np.concatenate([[0, t // 3, max(0, t - 700)] for t in want.total_samples.tolist()])
        lengths = np.array([1000, 2049, 900] * 3)
        a, na = got.decode_ranges(files, starts, lengths)
        b, nb = want.decode_ranges(files, starts, lengths)
        assert np.array_equal(na, nb) and torch.equal(a, b) and int(np.min(na)) > 0
    finally:
        got.close()
        want.close()
    with pytest.raises(v.VbmError, match="file 1: no Vorbis stream"):
        v.OggIndex([muxed[0], S.case6()["foreign alone"]], device_demux=device_demux, multiplexed=True)


# ---- stream order -------------------------------------------------------------------------------------------------------

def test_two_selectors_on_two_streams(cuda):
    """two selectors on two streams, three calls each back to back, every selection followed by the demux scan of its
    output on the same stream with no host wait in between: the third call reuses the pinned slot of the first"""
    batches = [[m for _, m, _ in S.singles()], S.alignment_files(), list(S.damage().values())[:11]]
    packed = [B.pack(blobs, first) for blobs, first in zip(batches, (0, 5, 11))]
    want = [S.expected(blobs) for blobs in batches]
    d_in = [torch.from_numpy(data.copy()).cuda() for data, _ in packed]
    nmax, bmax = max(len(b) for b in batches), max(len(d) for d, _ in packed)
    isz, fsz = S.info_dtype().itemsize, B._info_dtype().itemsize
    work = []
    for order in ([0, 1, 2], [2, 0, 1]):
        sel, dm, calls = S.Select("device", nmax, bmax), B.Batch("device", nmax, bmax), []
        for k in order:
            n, total = len(batches[k]), len(want[k][0])
            calls.append(dict(k=k, out=torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda"),
                              oo=torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                              info=torch.zeros(n * isz, dtype=torch.uint8, device="cuda"),
                              finfo=torch.zeros(n * fsz, dtype=torch.uint8, device="cuda"),
                              totals=torch.zeros(3, dtype=torch.int64, device="cuda")))
        work.append((sel, dm, calls, torch.cuda.Stream()))
    torch.cuda.synchronize()
    for step in range(3):
        for sel, dm, calls, q in work:
            c = calls[step]
            k = c["k"]
            n, total = len(batches[k]), len(want[k][0])
            with torch.cuda.stream(q):
                assert sel.select_raw(n, d_in[k].data_ptr(), packed[k][1].ctypes.data, c["out"].data_ptr(), total,
                                      c["oo"].data_ptr(), c["info"].data_ptr()) == 0
                # the offsets the selection will have written are the model's: nothing is read back for them
                assert dm.scan_raw(n, c["out"].data_ptr(), want[k][1].ctypes.data, c["finfo"].data_ptr(),
                                   c["totals"].data_ptr()) == 0
    torch.cuda.synchronize()
    ref = {}
    for sel, dm, calls, q in work:
        with torch.cuda.stream(q):
            assert sel.status() == 0
        for c in calls:
            k = c["k"]
            out, off, info = want[k]
            got = c["out"].cpu().numpy()
            assert got[:len(out)].tobytes() == out and (got[len(out):] == 0xA5).all(), k
            assert np.array_equal(c["oo"].cpu().numpy(), off)
            assert S.same_info(c["info"].cpu().numpy().view(S.info_dtype()), info)
            if k not in ref:
                h = B.Batch("host", nmax, bmax)
                ref[k] = h.scan(np.frombuffer(out, np.uint8), off)
                h.close()
            assert c["finfo"].cpu().numpy().tobytes() == ref[k][0].tobytes(), k
            assert np.array_equal(c["totals"].cpu().numpy(), ref[k][1])
        sel.close()
        dm.close()
