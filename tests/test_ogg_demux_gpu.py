"""Batch Ogg demux on the device (vbm_ogg_demux_scan / _fill): equal to its host twin on the corpora of the CPU file, info
structs included; the every-prefix batch; its output fed unchanged to Decoder.synthesis_runs; decode_ogg with
device_demux=True equal to decode_ogg bit for bit; two demuxers on two streams at once."""
import numpy as np
import pytest
import torch

from tests import ogg_demux_batch as B
from tests.ogg_demux_batch import ECAP, EOGG
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu

OUTPUTS = ("headers", "payload", "offsets", "granulepos", "eos")


def _same_as_twin(blobs, first=0):
    hinfo, htotals, hres = B.run("host", blobs, first)
    info, totals, res = B.run("device", blobs, first)
    assert res.status == 0 and res.canaries_ok
    assert np.array_equal(totals, htotals), (totals, htotals)
    assert np.array_equal(info.view(np.uint8), hinfo.view(np.uint8)), np.flatnonzero(info != hinfo)[:8]
    for name in OUTPUTS:
        got, want = getattr(res, name), getattr(hres, name)
        assert np.array_equal(got, want), f"{name}: first difference at {np.flatnonzero(got != want)[:4]}"
    return info, totals, res


def _alignment_batch():
    good = [b for _, b in B.directed()[1:7]] + [B.mixed()[1][1]]
    blobs = []
    for k, b in enumerate(good):
        blobs += [b"\xee" * (1 + k % 3), b]
    return blobs


@pytest.mark.parametrize("corpus", ["mixed", "mixed reversed", "directed", "no files", "failures only",
                                    "aligned 0", "aligned 1", "aligned 2", "aligned 3"])
def test_device_equals_host_twin(cuda, corpus):
    if corpus.startswith("aligned"):
        blobs, first = _alignment_batch(), int(corpus[-1])
    else:
        first = 0
        blobs = {"mixed": [b for _, b in B.mixed()], "mixed reversed": [b for _, b in B.mixed()][::-1],
                 "directed": [b for _, b in B.directed()], "no files": [],
                 "failures only": [b"", b"OggS", B.mixed()[0][1]]}[corpus]
    info, totals, res = _same_as_twin(blobs, first)
    B.check_csr(info, totals, res)
    if corpus == "mixed":                                   # and the yardstick itself, file by file
        for f, blob in enumerate(blobs):
            assert B.same(B.file_view(info, res, f), B.single(blob)), f


def test_every_prefix_as_one_batch(cuda):
    """adjacent files: a read past a file's end meets the next prefix and shows as a wrong result"""
    blob, bounds = B.six_packet_file()
    blobs = [blob[:k] for k in range(len(blob) + 1)]
    info, totals, res = _same_as_twin(blobs)
    ok = np.flatnonzero(info["status"] == 0).tolist()
    assert len(ok) >= 2 and set(ok) <= bounds
    for k in ok:
        assert B.same(B.file_view(info, res, k), B.single(blob[:k])), k


@pytest.mark.parametrize("short", ["packets", "payload", "headers"])
def test_capacity_one_short_writes_nothing(cuda, short):
    blobs = [b for _, b in B.mixed()[:6]]
    data, offsets = B.pack(blobs)
    b = B.Batch("device", len(blobs), len(data))
    try:
        info, totals = b.scan(data, offsets)
        res = b.fill(totals, short=short)
        assert res.status == ECAP and not res.touched and res.canaries_ok
        res = b.fill(totals)
        assert res.status == 0 and res.touched and res.canaries_ok
    finally:
        b.close()


@pytest.fixture(scope="module")
def encoded(cuda):
    """five real files of two header classes: stereo 44100 q5 (three lengths) and mono 8 kHz (two), each under 2 s"""
    import vorbis_aotuv_lancer_amd as v
    stereo = v.encode_ogg([synth_signal(2, 44100, n, seed=3 + i) for i, n in enumerate((70001, 30000, 4099))], 44100,
                          quality=0.5, serialnos=[11, 12, 13])
    mono = v.encode_ogg([synth_signal(1, 8000, n, seed=8 + i) for i, n in enumerate((15000, 2500))], 8000, quality=0.5,
                        serialnos=[21, 22])
    files = [stereo[0], mono[0], stereo[1], stereo[2], mono[1]]
    return files, v.decode_ogg(files)


def test_output_feeds_synthesis_runs_unchanged(cuda, encoded):
    """two stereo files as two runs of one call and a mono file, straight from the batch's tensors"""
    import vorbis_aotuv_lancer_amd as v
    files, want = encoded
    order = [0, 2, 1]                                        # stereo, stereo, mono: the stereo files adjacent in the CSR
    b = v.demux_ogg_device([files[i] for i in order])
    assert b.status == [0, 0, 0] and b.payload.is_cuda and b.offsets.is_cuda
    for members in ([0, 1], [2]):
        ds = v.DecodeSetup(b.headers[members[0]])
        dec = v.Decoder(ds, len(members), 4096)
        a = int(b.packet_base[members[0]])
        counts = [int(b.packets[f]) for f in members]
        P = sum(counts)
        pcm, run_samples, _, _ = dec.synthesis_runs(list(range(len(members))), counts, b.payload, b.offsets[a:a + P + 1],
                                                     granulepos=b.granulepos[a:a + P], eos=b.eos[a:a + P])
        n = run_samples.cpu().tolist()
        for r, f in enumerate(members):
            ref, rate = want[order[f]]
            assert rate == ds.rate and n[r] == ref.shape[1] > 0
            assert torch.equal(pcm[r, :, :n[r]], ref), (f, r)
        dec.close()
        ds.close()


def test_decode_ogg_with_device_demux(cuda, encoded):
    import vorbis_aotuv_lancer_amd as v
    files, want = encoded
    for mp in (4096, 37):
        got = v.decode_ogg(files, max_packets=mp, device_demux=True)
        assert len(got) == len(want)
        for i, ((a, ra), (b, rb)) in enumerate(zip(got, want)):
            assert ra == rb and a.shape == b.shape and torch.equal(a, b), (mp, i)
    bad = bytearray(files[2])
    bad[len(bad) // 2] ^= 1
    with pytest.raises(v.VbmError, match="file 3"):
        v.decode_ogg(files[:3] + [bytes(bad)] + files[3:], device_demux=True)


def test_two_demuxers_on_two_streams(cuda):
    """scan + fill of two batches enqueued on two streams with no wait in between: the bytes of each in sequence"""
    batches = [[b for _, b in B.mixed()], [b for _, b in B.directed()]]
    want = [B.run("host", blobs) for blobs in batches]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    work = []
    for blobs, (hinfo, htotals, _) in zip(batches, want):
        data, offsets = B.pack(blobs)
        P, nB, H = (int(x) for x in htotals)
        work.append(dict(b=B.Batch("device", len(blobs), len(data)), data=torch.from_numpy(data.copy()).cuda(), offsets=offsets,
                         info=torch.zeros(len(blobs) * hinfo.itemsize, dtype=torch.uint8, device="cuda"),
                         totals=torch.zeros(3, dtype=torch.int64, device="cuda"),
                         headers=torch.zeros(H, dtype=torch.uint8, device="cuda"),
                         payload=torch.zeros(nB, dtype=torch.uint8, device="cuda"),
                         offs=torch.zeros(P + 1, dtype=torch.int64, device="cuda"),
                         granulepos=torch.zeros(P, dtype=torch.int64, device="cuda"),
                         eos=torch.zeros(P, dtype=torch.uint8, device="cuda"), caps=(H, nB, P)))
    torch.cuda.synchronize()
    for w, q in zip(work, streams):
        with torch.cuda.stream(q):
            H, nB, P = w["caps"]
            assert w["b"].scan_raw(len(w["offsets"]) - 1, w["data"].data_ptr(), w["offsets"].ctypes.data, w["info"].data_ptr(),
                                   w["totals"].data_ptr()) == 0
            assert w["b"].fill_raw(w["headers"].data_ptr(), H, w["payload"].data_ptr(), nB, w["offs"].data_ptr(),
                                   w["granulepos"].data_ptr(), w["eos"].data_ptr(), P) == 0
    torch.cuda.synchronize()
    for w, q, (hinfo, htotals, hres) in zip(work, streams, want):
        with torch.cuda.stream(q):
            assert w["b"].status() == 0
        assert np.array_equal(w["totals"].cpu().numpy(), htotals)
        assert np.array_equal(w["info"].cpu().numpy(), hinfo.view(np.uint8))
        for name, key in zip(OUTPUTS, ("headers", "payload", "offs", "granulepos", "eos")):
            assert np.array_equal(w[key].cpu().numpy(), getattr(hres, name)), name
        w["b"].close()
    assert EOGG in want[0][0]["status"]
