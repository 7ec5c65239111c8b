"""Incremental Ogg demux on the device (vbm_ogg_feed_scan / _fill): every scenario of the CPU file equal to the host twin
call by call, info structs, totals and outputs; chunk and tail alignments; the live loop, OggFeed straight into
Decoder.synthesis_runs, equal to decode_ogg bit for bit; two feeds on two streams at once."""
import numpy as np
import pytest
import torch

from tests import ogg_feed_cases as F
from tests.ogg_demux_batch import mixed, six_packet_file
from tests.signals import synth_signal

pytestmark = pytest.mark.gpu


def _log(out):
    return out[0] if isinstance(out, tuple) else out


def _same_as_twin(scenario, *args):
    """the scenario's own assertions on the device, and then its whole log against the twin's"""
    dev, host = scenario("device", *args), scenario("host", *args)
    got, want = _log(dev), _log(host)
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a[0], [i for i, (x, y) in enumerate(zip(a, b)) if x != y])
    return dev, host


@pytest.mark.parametrize("cs", (None,) + F.CHUNKS)
def test_corpus_equals_host_twin(cuda, cs):
    dev, host = _same_as_twin(F.scenario_corpus, cs)
    assert dev[1] == host[1]


def test_every_cut_point_in_two_calls(cuda):
    _same_as_twin(F.scenario_every_cut)


def test_three_calls_at_random_cuts(cuda):
    _same_as_twin(F.scenario_random_cuts)


def test_one_byte_per_call(cuda):
    _same_as_twin(F.scenario_byte_by_byte)


@pytest.mark.parametrize("which", ["packet", "header", "page"])
def test_too_big_is_that_slots_alone(cuda, which):
    _same_as_twin(F.scenario_too_big, which)


@pytest.mark.parametrize("short", ["packets", "payload"])
def test_capacity_one_short_writes_nothing_and_keeps_the_state(cuda, short):
    _same_as_twin(F.scenario_capacity_short, short)


def test_reset_unlisted_and_empty_chunks(cuda):
    _same_as_twin(F.scenario_slots)


def test_argument_checks(cuda):
    F.check_einval("device")


@pytest.mark.parametrize("first", [0, 1, 2, 3])
def test_alignments(cuda, first):
    _same_as_twin(F.scenario_alignment, first)


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


def test_live_loop_into_synthesis_runs(cuda, encoded):
    """1000 bytes per file per call; each call's tensors go to synthesis_runs as they are"""
    import vorbis_aotuv_lancer_amd as v
    files, want = encoded
    for members in ([0, 2, 3], [1, 4]):                         # the stereo files, the mono files: one decoder each
        blobs = [files[i] for i in members]
        feed = v.OggFeed(len(blobs), 1000 * len(blobs), max_page_carry=8192)
        dec = ds = None
        pcm = [[] for _ in blobs]
        for ids, chunks, end in F.calls_of(blobs, 1000):
            r = feed.push(ids, chunks, end)
            assert r.payload.is_cuda and r.offsets.is_cuda and not any(r.status)
            live = np.flatnonzero(r.counts)
            if not len(live):
                continue
            if dec is None:
                ds = v.DecodeSetup(feed.headers(int(r.ids[live[0]])))
                dec = v.Decoder(ds, len(blobs), 4096)
            out, n, _, status = dec.synthesis_runs(r.ids[live], r.counts[live], r.payload, r.offsets, granulepos=r.granulepos,
                                                   eos=r.eos)
            assert not status.cpu().numpy().any()
            for row, (slot, k) in enumerate(zip(r.ids[live].tolist(), n.cpu().tolist())):
                pcm[slot].append(out[row, :, :k].clone())
        for slot, i in enumerate(members):
            assert feed.headers(slot) == v.demux_ogg(files[i])[0], i
            ref, rate = want[i]
            got = torch.cat(pcm[slot], dim=1)
            assert rate == ds.rate and got.shape == ref.shape and torch.equal(got, ref), i
        feed.close()
        dec.close()
        ds.close()


def test_two_feeds_on_two_streams(cuda):
    """every call of two feeds enqueued on two streams with no wait in between: the bytes of each alone"""
    jobs = [([six_packet_file()[0], dict(mixed())["small_packets"]], 30000),
            ([b for _, b in mixed()[:6]], 100000)]
    work = []
    for blobs, cs in jobs:
        host = F.Feed("host", len(blobs), cs * len(blobs))
        F.feed_all(host, blobs, cs)
        host.close()
        calls = F.calls_of(blobs, cs)
        scans, fills = [e for e in host.log if e[0] == "scan"], [e for e in host.log if e[0] == "fill"]
        assert len(scans) == len(fills) == len(calls) >= 3
        bufs = []
        for (ids, chunks, end), (_, info, totals) in zip(calls, scans):
            P, nB = totals
            off = np.zeros(len(ids) + 1, np.int64)
            np.cumsum([len(c) for c in chunks], out=off[1:])
            bufs.append(dict(ids=np.array(ids, np.int32), off=off, end=np.array(end, np.uint8),
                             data=torch.from_numpy(np.frombuffer(b"".join(chunks), np.uint8).copy()).cuda(),
                             meta=torch.zeros(16 + len(info), dtype=torch.uint8, device="cuda"),
                             payload=torch.zeros(nB, dtype=torch.uint8, device="cuda"),
                             offsets=torch.zeros(P + 1, dtype=torch.int64, device="cuda"),
                             granulepos=torch.zeros(P, dtype=torch.int64, device="cuda"),
                             eos=torch.zeros(P, dtype=torch.uint8, device="cuda"), caps=(nB, P)))
        work.append(dict(feed=F.Feed("device", len(blobs), cs * len(blobs)), bufs=bufs, scans=scans, fills=fills))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for j in range(max(len(w["bufs"]) for w in work)):
        for w, q in zip(work, streams):
            if j >= len(w["bufs"]):
                continue
            b = w["bufs"][j]
            with torch.cuda.stream(q):
                assert w["feed"].scan_raw(len(b["ids"]), b["ids"].ctypes.data, b["data"].data_ptr(), b["off"].ctypes.data,
                                          b["end"].ctypes.data, b["meta"].data_ptr() + 16, b["meta"].data_ptr()) == 0
                assert w["feed"].fill_raw(b["payload"].data_ptr(), b["caps"][0], b["offsets"].data_ptr(),
                                          b["granulepos"].data_ptr(), b["eos"].data_ptr(), b["caps"][1]) == 0
    torch.cuda.synchronize()
    for w, q in zip(work, streams):
        with torch.cuda.stream(q):
            assert w["feed"].status() == 0
        for b, (_, info, totals), fill in zip(w["bufs"], w["scans"], w["fills"]):
            meta = b["meta"].cpu().numpy()
            assert meta[:16].view(np.int64).tolist() == totals and meta[16:].tobytes() == info
            assert b["payload"].cpu().numpy().tobytes() == fill[4] and b["offsets"].cpu().tolist() == fill[5]
            assert b["granulepos"].cpu().tolist() == fill[6] and b["eos"].cpu().tolist() == fill[7]
        w["feed"].close()
