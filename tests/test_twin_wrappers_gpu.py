"""The wrapper classes of stream.py, device form against host=True form, field for field: each states its call once for
both forms (_twin._TwinHandle._call), and the CPU suite runs only the host one.  The batches are the smallest that can
go wrong: no file at all (every optional address None), one empty file beside one real file of a few pages, and for the
feed one slot pushed in two cuts, with and without resync."""
import numpy as np
import pytest
import torch

import vorbis_aotuv_lancer_amd as v
from tests.ogg_chain_cases import two_link_file
from tests.ogg_demux_batch import six_packet_file
from tests.ogg_select_cases import case1

pytestmark = pytest.mark.gpu

BATCHES = {"no file": lambda: [], "an empty file beside a real one": lambda: [b"", six_packet_file()[0]]}


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same(d, h, fields):
    for name in fields:
        x, y = _np(getattr(d, name)), _np(getattr(h, name))
        if isinstance(y, np.ndarray):
            assert type(x) is type(y) and x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
        else:
            assert x == y, name


BATCH = ("names", "status", "headers", "info", "payload", "offsets", "granulepos", "eos", "file_links", "gap", "events",
         "select_info")
RESULT = ("ids", "info", "counts", "status", "payload", "offsets", "granulepos", "eos", "gap", "events", "left", "link",
          "link_started")


def _pair(cls, *args, **kw):
    return cls(*args, **kw), cls(*args, host=True, **kw)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("cls", [v.DeviceDemuxer, v.ResyncDemuxer])
def test_batch_demuxers(cuda, cls, batch):
    blobs = BATCHES[batch]()
    with cls(2, 1 << 16) as d, cls(2, 1 << 16, host=True) as h:
        bd, bh = d.demux(blobs), h.demux(blobs)
        assert torch.is_tensor(bd.payload) and bd.payload.device == d.device and isinstance(bh.payload, np.ndarray)
        _same(bd, bh, BATCH)
        assert len(bd) == (len(blobs) // 2 if cls is v.ResyncDemuxer else len(blobs))


def test_resync_demuxer_retries_on_the_device_as_on_the_host(cuda):
    chain = [b"".join(two_link_file())]
    with v.ResyncDemuxer(1, 1 << 16) as d, v.ResyncDemuxer(1, 1 << 16, host=True) as h:
        got, want = (rd._scan(1, *rd.mem.join(chain), 1) for rd in (d, h))      # room for one entry of two
        assert int(want[0][5]) == h.ECAP and [x.tobytes() for x in got] == [y.tobytes() for y in want]
        bd, bh = (rd.demux_joined(["f"], *rd.mem.join(chain), entry_cap=1) for rd in (d, h))
        _same(bd, bh, BATCH)
        assert len(bd) == 2


@pytest.mark.parametrize("batch", list(BATCHES) + ["a chain of two links"])
def test_chain_splitter(cuda, batch):
    blobs = [b"".join(two_link_file())] if batch not in BATCHES else BATCHES[batch]()
    with v.ChainSplitter(2, 1 << 16) as d, v.ChainSplitter(2, 1 << 16, host=True) as h:
        for cap in (None, 0):                                 # 0: the second try, with the total the first counted
            got, want = (sp.split(*sp.mem.join(blobs), link_cap=cap) for sp in (d, h))
            for x, y in zip(got, want):
                assert x.dtype == y.dtype and x.tolist() == y.tolist()
        assert len(want[1]) - 1 == (2 if batch not in BATCHES else len(blobs))


@pytest.mark.parametrize("batch", list(BATCHES) + ["a multiplexed file"])
def test_stream_selector(cuda, batch):
    blobs = [case1()["skeleton first"][0], b""] if batch not in BATCHES else BATCHES[batch]()
    with v.StreamSelector(2, 1 << 16) as d, v.StreamSelector(2, 1 << 16, host=True) as h:
        got, want = (s.select(*s.mem.join(blobs)) for s in (d, h))
    assert torch.is_tensor(got[0]) and isinstance(want[0], np.ndarray)
    for x, y in zip(got, want):
        assert _np(x).dtype == y.dtype and _np(x).tobytes() == y.tobytes()
    if batch not in BATCHES:
        assert want[0].tobytes() == case1()["skeleton first"][1] and want[2]["foreign_pages"][0] > 0


@pytest.mark.parametrize("flags", [{}, {"chained": True}, {"multiplexed": True}, {"chained": True, "multiplexed": True},
                                   {"resync": True}], ids=lambda f: "+".join(f) or "plain")
def test_demux_ogg_device_one_shots(cuda, flags):
    blobs = [b"", b"".join(two_link_file()) if flags.get("chained") or flags.get("resync") else six_packet_file()[0]]
    _same(v.demux_ogg_device(blobs, **flags), v.demux_ogg_device(blobs, host=True, **flags), BATCH)


@pytest.mark.parametrize("resync", [False, True])
def test_feed_one_slot_in_two_cuts(cuda, resync):
    blob = six_packet_file()[0]
    cut = len(blob) // 2 + 7
    d, h = _pair(v.OggFeed, 2, 1 << 16, resync=resync)
    with d, h:
        _same(d.push([], []), h.push([], []), RESULT)         # no slot: every optional address None
        for part, end in ((blob[:cut], False), (blob[cut:], True)):
            rd, rh = d.push([1], [part], end=end), h.push([1], [part], end=end)
            assert torch.is_tensor(rd.payload) and rd.payload.device == d.device and isinstance(rh.payload, np.ndarray)
            _same(rd, rh, RESULT)
        assert d.headers(1) == h.headers(1) == v.demux_ogg(blob)[0]
        assert (rh.gap is not None) == resync and (rh.events is not None) == resync


def test_feed_push_all_gathers_what_came_back(cuda):
    """a chain pushed whole: a resync feed stops at the second link and gives the rest back, which push_all gathers out of
    the one buffer, on the device with torch indexing and on the host with numpy's"""
    blobs = [b"".join(two_link_file()), six_packet_file()[0]]
    d, h = _pair(v.OggFeed, 2, 1 << 16, resync=True)
    with d, h:
        got, want = ([r for r in f.push_all([0, 1], f.mem.join(blobs)[0], end=True, offsets=f.mem.join(blobs)[1])]
                     for f in (d, h))
        assert len(got) == len(want) >= 2
        for rd, rh in zip(got, want):
            _same(rd, rh, RESULT)
