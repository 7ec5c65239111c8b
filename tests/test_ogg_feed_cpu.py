"""Incremental Ogg demux, host twin (vbm_host_ogg_feed_*): streams pushed in chunks of any size come out as vbm_ogg_demux
gives the whole file; violations, the three capacities, fill capacities, slot handling and argument checks; no read past
a chunk's end.  Host only: runs without a GPU.  The scenarios are in tests/ogg_feed_cases.py."""
import ctypes as C
import mmap

import numpy as np
import pytest

from tests import ogg_feed_cases as F
from tests.ogg_demux_batch import EOGG, single, six_packet_file
from tests.ogg_pages import guarded_mapping


@pytest.fixture(scope="module")
def whole_push():
    """what every file of the corpus delivers when it is pushed whole, with `end`"""
    return F.scenario_corpus("host", None)[1]


def test_corpus_pushed_whole(whole_push):
    files = F.corpus()
    assert sum(want is not None for _, _, want in files) >= 10 and sum(want is None for _, _, want in files) >= 12
    for name, _, want in files:
        assert (whole_push[name][0] == EOGG) == (want is None), name


@pytest.mark.parametrize("cs", F.CHUNKS)
def test_corpus_at_any_cut(whole_push, cs):
    """good files equal vbm_ogg_demux's output, rejected ones end as VBM_EOGG (asserted in the scenario); status and
    delivered packets of every file are those of the whole push"""
    _, delivered = F.scenario_corpus("host", cs)
    for name, got in delivered.items():
        assert got == whole_push[name], name


def test_every_cut_point_in_two_calls():
    F.scenario_every_cut("host")


def test_three_calls_at_random_cuts():
    F.scenario_random_cuts("host")


def test_one_byte_per_call():
    F.scenario_byte_by_byte("host")


@pytest.mark.parametrize("which", ["packet", "header", "page"])
def test_too_big_is_that_slots_alone(which):
    F.scenario_too_big("host", which)


@pytest.mark.parametrize("short", ["packets", "payload"])
def test_capacity_one_short_writes_nothing_and_keeps_the_state(short):
    F.scenario_capacity_short("host", short)


def test_reset_unlisted_and_empty_chunks():
    F.scenario_slots("host")


def test_argument_checks():
    F.check_einval("host")


def test_oggfeed_class_on_the_host():
    """OggFeed(host=True): push / headers / reset / close over the same calls"""
    import vorbis_aotuv_lancer_amd as v
    blob, _ = six_packet_file()
    want = single(blob)
    feed = v.OggFeed(2, 2 * len(blob), max_page_carry=8192, host=True)
    st = F.Streams()
    for a in range(0, len(blob), 1000):
        r = feed.push([1, 0], [blob[a:a + 1000]] * 2, end=a + 1000 >= len(blob))
        assert isinstance(r.payload, np.ndarray) and r.counts.tolist() == r.info["packets"].tolist()
        st.add([1, 0], r.info, r)
    assert st.status == {0: 0, 1: 0}
    for k in (0, 1):
        h = feed.headers(k)
        assert [len(x) for x in h] == want[0] and b"".join(h) == want[1]
        pay, offs, gp, eos = st.packets(k)
        assert (pay, offs, gp, eos) == (want[2], want[3].tolist(), want[4].tolist(), want[5].tolist())
    feed.reset([0])
    with pytest.raises(v.VbmError):
        feed.headers(0)
    assert len(feed.headers(1)) == 3
    with pytest.raises(v.VbmError):
        feed.push([0, 0], [b"", b""])
    feed.close()


def test_feed_never_reads_past_a_chunk():
    """every prefix of a valid file as ONE chunk whose last byte is the last readable byte, and then the rest placed
    the same way: the twin reads only the chunk's bytes; none faults, and the stream comes out whole"""
    blob, _ = six_packet_file()
    want = single(blob)
    lib = F._lib()
    libc = C.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    m, base, cap = guarded_mapping(libc, len(blob))
    feed = F.Feed("host", 1, len(blob), carry=8192)
    info = np.zeros(1, F._info_dtype())
    totals = np.zeros(2, np.int64)
    ids = np.zeros(1, np.int32)
    end = np.zeros(1, np.uint8)
    try:
        for n in range(0, len(blob) + 1, 7):
            feed.reset([0])
            got = []
            for piece, last in ((blob[:n], 0), (blob[n:], 1)):
                at = base + cap - len(piece)
                C.memmove(at, piece, len(piece))
                off = np.array([0, len(piece)], np.int64)
                end[0] = last
                assert lib.vbm_host_ogg_feed_scan(feed.h, 1, ids.ctypes.data, C.c_void_p(at), off.ctypes.data,
                                                  end.ctypes.data, info.ctypes.data, totals.ctypes.data) == 0
                got.append(feed.fill(totals).payload.tobytes())
            assert info[0]["status"] == 0 and b"".join(got) == want[2], n
    finally:
        libc.mprotect(C.c_void_p(base + cap), C.c_size_t(mmap.PAGESIZE), 3)
        m.close()
        feed.close()
