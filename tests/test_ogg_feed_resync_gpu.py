"""The resync mode of the Ogg feed on the device (k_feed_resync_walk and the kernels it shares with the strict mode): the
scenarios of the CPU file with slots of different fates in one call, every call equal to the host twin in its info and
event structs, totals, CSR and gap marks, and equal to the byte-serial model."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ogg_chain_cases as CH
from tests import ogg_feed_resync_cases as R
from tests.ogg_demux_batch import six_packet_file

pytestmark = pytest.mark.gpu


def fates():
    """one stream per fate: undamaged, chained, a lost page, a lost pair, a mid-stream join, damage, garbage, a false
    header, a page lost while the headers are open, foreign pages and pages after the end, a truncated page that claims
    more bytes than follow"""
    six, ps = R.paged_six(), R.pages(R.paged_six())
    ap = R.audio_pages(six)
    a, b, c = CH.small_links(3)
    foreign = R.pages(CH.reserial(six, 555))
    return [six_packet_file()[0], six, a + b + c, R.without_pages(six, {ap[2]}), R.without_pages(six, {ap[1], ap[2]}),
            R.without_pages(six, set(ap[:3])), R.flip(six, ap[3], "body"), R.flip(six, ap[0], "lacing"),
            R.join(ps[:4]) + bytes(range(1, 200)) + R.join(ps[4:]), R.false_capture_file()[0],
            ps[0] + R.join(ps[2:]) + b, R.join(ps[:3]) + foreign[4] + R.join(ps[3:]) + foreign[5] + ps[-1],
            R.join(R.pages(R.long_file())[:12]), R.without_pages(R.long_file(), {9}), six[:-9], R.overclaim_file()[0]]


def both(blobs, cuts, **kw):
    dev, host = R.Run("device", blobs, cuts, **kw), R.Run("host", blobs, cuts, **kw)
    assert len(dev.log) == len(host.log)
    for k, (a, b) in enumerate(zip(dev.log, host.log)):
        assert a == b, (k, [i for i, (x, y) in enumerate(zip(a, b)) if x != y])
    assert dev.headers == host.headers and dev.status == host.status
    return dev


@pytest.mark.parametrize("step", (0, 27, 255, 4096))
def test_fates_in_one_call_equal_twin_and_model(cuda, step):
    blobs = fates()
    cuts = [R.cuts_every(len(b), step) if step else [] for b in blobs]
    if step == 27:                                       # the short streams only: a few hundred calls
        blobs, cuts = zip(*[(b, c) for b, c in zip(blobs, cuts) if len(b) < 9000])
    R.check_against_model(both(list(blobs), list(cuts)), blobs, cuts)


@pytest.mark.parametrize("first", (0, 1, 2, 3))
def test_alignments(cuda, first):
    """the chunks start `first` bytes into the buffer; the odd max_page_carry puts the tails of slots 0..3 and the runs of
    the work buffer at every alignment"""
    blobs = fates()[1:9]
    cuts = [R.cuts_every(len(b), 101 + 2 * k) for k, b in enumerate(blobs)]
    R.check_against_model(both(blobs, cuts, first=first, max_page_carry=65307 - 2 * first), blobs, cuts)


def test_65_slots(cuda):
    """one slot past 16 workgroups of four wavefronts"""
    links = CH.small_links(65)
    blobs = [links[k] + links[(k + 1) % 65] if k % 3 == 0 else R.without_pages(links[k], {2}) if k % 3 == 1 else links[k]
             for k in range(65)]
    cuts = [[len(b) // 3, 2 * len(b) // 3 + k % 5] for k, b in enumerate(blobs)]
    R.check_against_model(both(blobs, cuts), blobs, cuts)


def test_two_feeds_on_two_streams(cuda):
    """every call of two resync feeds enqueued on two streams with no wait in between: the bytes of each alone"""
    from vorbis_aotuv_lancer_amd._lib import lib
    from vorbis_aotuv_lancer_amd.stream import FEED_EVENTS, FEED_INFO
    jobs = [(fates()[1:6], 300), (fates()[6:12], 1000)]
    work = []
    for blobs, step in jobs:
        host = R.Run("host", blobs, [R.cuts_every(len(b), step) for b in blobs])
        feed = R.make_feed("device", len(blobs), step * len(blobs))
        bufs = []
        for (ids, raw, off, end), want in zip(host.inputs, host.log):
            n, P, B = len(ids), len(want[5]) // 8, len(want[3])
            bufs.append(dict(ids=ids, off=off, end=end, data=torch.from_numpy(raw).cuda(), P=P, B=B, want=want,
                             meta=torch.zeros(16 + n * (FEED_INFO.itemsize + FEED_EVENTS.itemsize), dtype=torch.uint8, device="cuda"),
                             payload=torch.zeros(B, dtype=torch.uint8, device="cuda"),
                             offsets=torch.zeros(P + 1, dtype=torch.int64, device="cuda"),
                             granulepos=torch.zeros(P, dtype=torch.int64, device="cuda"),
                             eos=torch.zeros(P, dtype=torch.uint8, device="cuda"),
                             gap=torch.zeros(P, dtype=torch.uint8, device="cuda")))
        work.append(dict(feed=feed, bufs=bufs))
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for j in range(max(len(w["bufs"]) for w in work)):
        for w, q in zip(work, streams):
            if j >= len(w["bufs"]):
                continue
            b, h, s = w["bufs"][j], w["feed"]._h, C.c_void_p(q.cuda_stream)
            n, m = len(b["ids"]), b["meta"].data_ptr()
            assert lib.vbm_ogg_feed_scan(h, n, b["ids"].ctypes.data, b["data"].data_ptr(), b["off"].ctypes.data,
                                         b["end"].ctypes.data, m + 16, m, s) == 0
            assert lib.vbm_ogg_feed_scan_events(h, m + 16 + n * FEED_INFO.itemsize, s) == 0
            assert lib.vbm_ogg_feed_fill_gaps(h, b["payload"].data_ptr(), b["B"], b["offsets"].data_ptr(),
                                              b["granulepos"].data_ptr(), b["eos"].data_ptr(), b["gap"].data_ptr(), b["P"],
                                              s) == 0
    torch.cuda.synchronize()
    for w in work:
        for k, b in enumerate(w["bufs"]):
            n, meta = len(b["ids"]), b["meta"].cpu().numpy()
            ni = n * FEED_INFO.itemsize
            got = (b["ids"].tobytes(), meta[16:16 + ni].tobytes(), meta[16 + ni:].tobytes()) + \
                tuple(b[x].cpu().numpy().tobytes() for x in ("payload", "offsets", "granulepos", "eos", "gap"))
            assert got == b["want"], k
            assert meta[:16].view(np.int64).tolist() == [b["P"], b["B"]]
        w["feed"].close()


def test_fill_one_short_then_again_and_strict_feeds(cuda):
    from vorbis_aotuv_lancer_amd._lib import lib
    from vorbis_aotuv_lancer_amd.stream import FEED_EVENTS, FEED_INFO
    import vorbis_aotuv_lancer_amd as v
    ps, ap = R.pages(R.paged_six()), R.audio_pages(R.paged_six())
    front, blob = R.join(ps[:ap[1]]), R.join(ps[ap[2]:])
    ref = R.make_feed("host", 1, len(front) + len(blob))
    ref.push([0], [front])
    want = ref.push([0], [blob])
    ref.close()
    feed = R.make_feed("device", 1, len(front) + len(blob))
    assert feed.push([0], [front]).counts[0] == 1
    P, B = len(want.granulepos), len(want.payload)
    ids, off = np.zeros(1, np.int32), np.array([0, len(blob)], np.int64)
    raw = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    meta = torch.zeros(16 + FEED_INFO.itemsize + FEED_EVENTS.itemsize, dtype=torch.uint8, device="cuda")
    q = feed._q()
    assert lib.vbm_ogg_feed_scan(feed._h, 1, ids.ctypes.data, raw.data_ptr(), off.ctypes.data, None, meta.data_ptr() + 16,
                                 meta.data_ptr(), q) == 0
    assert lib.vbm_ogg_feed_scan_events(feed._h, meta.data_ptr() + 16 + FEED_INFO.itemsize, q) == 0
    assert meta[:16].cpu().numpy().view(np.int64).tolist() == [P, B] and P == 4
    for pcap, bcap in ((P - 1, B), (P, B - 1), (P, B)):
        pay, offs = torch.full((B,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((P + 1,), -7, dtype=torch.int64, device="cuda")
        gp, eos = torch.full((P,), -7, dtype=torch.int64, device="cuda"), torch.full((P,), 0xEE, dtype=torch.uint8, device="cuda")
        gap = torch.full((P,), 0xEE, dtype=torch.uint8, device="cuda")
        assert lib.vbm_ogg_feed_fill_gaps(feed._h, pay.data_ptr(), bcap, offs.data_ptr(), gp.data_ptr(), eos.data_ptr(),
                                          gap.data_ptr(), pcap, q) == 0
        st = C.c_int(-7)
        assert lib.vbm_ogg_feed_status(feed._h, C.byref(st), q) == 0
        if (pcap, bcap) != (P, B):
            assert st.value == R.ECAP and bool((gap == 0xEE).all()) and bool((pay == 0xEE).all()) and bool((offs == -7).all())
        else:
            assert st.value == 0
            for got, w in ((pay, want.payload), (offs, want.offsets), (gp, want.granulepos), (eos, want.eos), (gap, want.gap)):
                assert np.array_equal(got.cpu().numpy(), w)
    assert want.gap.tolist() == [1, 0, 0, 0]
    feed.close()
    # a strict feed: no events, and fill_gaps writes zeros; the old fill on a resync feed drops the marks
    st = v.OggFeed(1, len(front) + len(blob))
    r = st.push([0], [front])
    assert r.gap is None and r.events is None
    ev = torch.zeros(FEED_EVENTS.itemsize, dtype=torch.uint8, device="cuda")
    assert lib.vbm_ogg_feed_scan_events(st._h, ev.data_ptr(), st._q()) == R.EINVAL
    st.close()
    assert lib.vbm_ogg_feed_scan_events(None, ev.data_ptr(), None) == R.EINVAL
