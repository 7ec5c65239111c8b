"""The split of chained Ogg files on the device (vbm_ogg_chain_split): equal to its host twin and to the page walker on the
corpora of the CPU file, every link demuxed on the device as vbm_ogg_demux demuxes its bytes alone; two splitters on two
streams at once; demux_ogg_device(chained=True) against its host twin; decode_ogg(chained=True) bit-equal to decode_ogg
of each link alone."""
import numpy as np
import pytest
import torch

from tests import ogg_chain_cases as K
from tests import ogg_demux_batch as B
from tests.ogg_chain_cases import ECAP
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu


def _corpus(name):
    a, b, _ = K.small_links(3)
    if name.startswith("aligned"):
        return K.alignment_batch(), int(name[-1])
    return {"chains": [x for x, _ in K.chains().values()], "corrupted middle links": list(K.middle_corruptions().values()),
            "no files": [], "empty and short": [b"", b"OggS" + b"\0" * 22, a + b, b""], "1025 files": K.many_files()}[name], 0


@pytest.mark.parametrize("corpus", ["chains", "corrupted middle links", "no files", "empty and short", "1025 files"] +
                         [f"aligned {k}" for k in range(8)])
def test_device_equals_host_twin(cuda, corpus):
    blobs, first = _corpus(corpus)
    hfl, hlo = K.run("host", blobs, first)
    fl, lo = K.run("device", blobs, first)
    assert np.array_equal(fl, hfl) and np.array_equal(lo, hlo)
    if corpus == "1025 files":
        K.check_split("device", blobs, first)
        return
    ok = K.check_demux("device", blobs, first)               # the walker, and vbm_ogg_demux link by link
    if corpus == "corrupted middle links":
        assert ok == [x for name in K.middle_corruptions() for x in K.MIDDLE[name]]
    if corpus == "chains":
        assert len(ok) == sum(n for _, n in K.chains().values())


def test_every_prefix_of_a_two_link_file_as_one_batch(cuda):
    """adjacent files: a read past a file's end meets the next prefix and shows as a wrong result"""
    l0, l1 = K.two_link_file()
    blob = l0 + l1
    blobs = [blob[:k] for k in range(len(blob) + 1)]
    hfl, hlo = K.run("host", blobs)
    fl, lo = K.run("device", blobs)
    assert np.array_equal(fl, hfl) and np.array_equal(lo, hlo)
    assert fl[-1] == 2 * len(blobs) - len(l0) - len(K.split_pages(l1)[0])
    # the links of the prefixes that reach into link 1, demuxed on the device and on the host twin
    j0, data = int(fl[len(l0) + 1]), np.frombuffer(b"".join(blobs), np.uint8)
    sub = lo[j0:]
    got = []
    for impl in ("host", "device"):
        b = B.Batch(impl, len(sub) - 1, int(sub[-1] - sub[0]))
        try:
            info, totals = b.scan(data, sub)
            got.append((info, b.fill(totals)))
        finally:
            b.close()
    (hinfo, hres), (info, res) = got
    assert np.array_equal(info.view(np.uint8), hinfo.view(np.uint8))
    for name in ("headers", "payload", "offsets", "granulepos", "eos"):
        assert np.array_equal(getattr(res, name), getattr(hres, name)), name
    whole = B.single(l0)
    for j in range(0, len(sub) - 1, 97):                     # the twin is pinned link by link in the CPU file
        link = data[int(sub[j]):int(sub[j + 1])].tobytes()
        assert B.same(B.file_view(info, res, j), whole if link == l0 else B.single(link)), j


def test_capacity_one_short_writes_nothing(cuda):
    blobs = [b for b, _ in K.chains().values()]
    data, offsets = B.pack(blobs)
    want_fl, want_lo = K.expected(blobs)
    total = int(want_fl[-1])
    c = K.Chain("device", len(blobs), len(data))
    try:
        r = c.split(data, offsets, total - 1)
        assert r.status == ECAP and not r.touched and r.canaries_ok
        assert np.array_equal(r.file_links, want_fl)
        r = c.split(data, offsets, total)
        assert r.status == 0 and r.touched and r.canaries_ok
        assert np.array_equal(r.file_links, want_fl) and np.array_equal(r.link_offsets, want_lo)
    finally:
        c.close()


def test_device_call_refuses_a_host_object_and_bad_arguments(cuda):
    data, offsets = B.pack(list(K.small_links(3)))
    d = torch.from_numpy(data.copy()).cuda()
    out = torch.zeros(16, dtype=torch.int64, device="cuda")
    host, dev = K.Chain("host", 3, len(data)), K.Chain("device", 3, len(data))
    try:
        host.impl, dev.impl = "device", "host"               # each call form with the other kind of object
        assert host.split_raw(3, d.data_ptr(), offsets.ctypes.data, out.data_ptr(), out.data_ptr() + 32, 8) == K.EINVAL
        assert dev.split_raw(3, data.ctypes.data, offsets.ctypes.data, out.data_ptr(), out.data_ptr() + 32, 8) == K.EINVAL
    finally:
        host.impl, dev.impl = "host", "device"
        host.close()
        dev.close()
    c = K.Chain("device", 3, len(data))
    try:
        ptrs = (d.data_ptr(), offsets.ctypes.data, out.data_ptr(), out.data_ptr() + 32)
        assert c.split_raw(4, *ptrs, 8) == K.EINVAL
        assert c.split_raw(3, *ptrs, -1) == K.EINVAL
        for k in range(4):
            assert c.split_raw(3, *ptrs[:k], None, *ptrs[k + 1:], 8) == K.EINVAL
        bad = offsets.copy()
        bad[3] += 1
        assert c.split_raw(3, d.data_ptr(), bad.ctypes.data, out.data_ptr(), out.data_ptr() + 32, 8) == K.EINVAL
        assert c.split_raw(3, *ptrs, 8) == 0 and c.status() == 0
        assert out.cpu().numpy()[:8].tolist() == [0, 1, 2, 3] + offsets.tolist()
    finally:
        c.close()


def test_two_splitters_on_two_streams(cuda):
    """two batches enqueued on two streams with no wait in between"""
    batches = [[x for x, _ in K.chains().values()], list(K.middle_corruptions().values())]
    want = [K.expected(blobs) for blobs in batches]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    work = []
    for blobs, (wfl, wlo) in zip(batches, want):
        data, offsets = B.pack(blobs)
        work.append(dict(c=K.Chain("device", len(blobs), len(data)), data=torch.from_numpy(data.copy()).cuda(), offsets=offsets,
                         fl=torch.zeros(len(wfl), dtype=torch.int64, device="cuda"),
                         lo=torch.zeros(len(wlo), dtype=torch.int64, device="cuda")))
    torch.cuda.synchronize()
    for w, q in zip(work, streams):
        with torch.cuda.stream(q):
            assert w["c"].split_raw(len(w["offsets"]) - 1, w["data"].data_ptr(), w["offsets"].ctypes.data, w["fl"].data_ptr(),
                                    w["lo"].data_ptr(), len(w["lo"]) - 1) == 0
    torch.cuda.synchronize()
    for w, q, (wfl, wlo) in zip(work, streams, want):
        with torch.cuda.stream(q):
            assert w["c"].status() == 0
        assert np.array_equal(w["fl"].cpu().numpy(), wfl) and np.array_equal(w["lo"].cpu().numpy(), wlo)
        w["c"].close()


def test_demux_ogg_device_chained_equals_its_host_twin(cuda):
    import vorbis_aotuv_lancer_amd as v
    a, b, c = K.small_links(3)
    files = [x for x, _ in K.chains().values()] + [b"", a] + list(K.middle_corruptions().values())[:4]
    h = v.demux_ogg_device(files, host=True, chained=True)
    d = v.demux_ogg_device(files, chained=True)
    assert d.payload.is_cuda and d.offsets.is_cuda and d.file_links.dtype == np.int64
    assert np.array_equal(d.file_links, h.file_links)
    assert d.file_links[-1] == len(d) > 2 * len(files) + 62     # more links than the first try has room for
    assert d.names == h.names and d.names[1] == "file 1 link 0" and d.names[2] == "file 1 link 1"
    assert [list(d.links(f)) for f in range(len(files))] == [list(h.links(f)) for f in range(len(files))]
    assert d.status == h.status and d.headers == h.headers
    assert np.array_equal(d.info.view(np.uint8), h.info.view(np.uint8))
    for name in ("payload", "offsets", "granulepos", "eos"):
        assert np.array_equal(getattr(d, name).cpu().numpy(), getattr(h, name)), name


@pytest.fixture(scope="module")
def encoded(cuda):
    """links of 0.2 to 0.5 s in two classes, dealt into two files of two and three links with one link in both; and
    every link decoded alone"""
    import vorbis_aotuv_lancer_amd as v
    stereo = v.encode_ogg([synth_signal(2, 44100, n, seed=50 + i) for i, n in enumerate((22050, 9000, 13001))], 44100,
                          quality=0.5, serialnos=[31, 32, 33])
    mono = v.encode_ogg([synth_signal(1, 8000, n, seed=60 + i) for i, n in enumerate((4000, 1700))], 8000, quality=0.5,
                        serialnos=[41, 42])
    files = [[stereo[0], mono[0]], [mono[1], stereo[0], stereo[2]]]
    alone = {half: [v.decode_ogg(links, halfrate=half) for links in files] for half in (False, True)}
    return files, alone, stereo[1]


@pytest.mark.parametrize("device_demux", [False, True])
@pytest.mark.parametrize("halfrate", [False, True])
def test_decode_ogg_chained(cuda, encoded, device_demux, halfrate):
    import vorbis_aotuv_lancer_amd as v
    files, alone, _ = encoded
    got = v.decode_ogg([b"".join(links) for links in files], chained=True, device_demux=device_demux, halfrate=halfrate)
    assert [len(g) for g in got] == [2, 3]
    for f, links in enumerate(got):
        for k, (pcm, rate) in enumerate(links):
            ref, ref_rate = alone[halfrate][f][k]
            assert rate == ref_rate and pcm.shape == ref.shape and pcm.shape[1] > 0 and torch.equal(pcm, ref), (f, k)
    assert got[0][0][1] == (22050 if halfrate else 44100) and got[0][1][1] == (4000 if halfrate else 8000)


@pytest.mark.parametrize("device_demux", [False, True])
def test_decode_ogg_chained_names_the_bad_link(cuda, encoded, device_demux):
    import vorbis_aotuv_lancer_amd as v
    files, _, spare = encoded
    bad = bytearray(spare)
    bad[len(bad) // 2] ^= 1
    chain = files[1][0] + files[1][1] + bytes(bad) + files[1][2]
    with pytest.raises(v.VbmError, match="file 1 link 2"):
        v.decode_ogg([b"".join(files[0]), chain], chained=True, device_demux=device_demux)
    got = v.decode_ogg([b"".join(files[0]), files[1][0] + spare], chained=True, device_demux=device_demux, max_packets=37)
    assert [len(g) for g in got] == [2, 2]
