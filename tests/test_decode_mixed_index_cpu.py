"""The host side of range stores and the index over several header classes, no device: vbm_host_decode_index_scan_mixed
(the CPU twin of the index kernels on a MixedDecoder) against vbm_host_decode_index_scan of each stream alone with its
class's setup, and the header grouping of OggIndex(one_decoder=True)."""
import numpy as np
import pytest

from tests import decode_mixed_range_cases as R
from tests.decode_packets import EINVAL


@pytest.fixture(scope="module")
def corpus():
    import vorbis_aotuv_lancer_amd as v
    classes, streams = R.index_streams()
    ds = [v.DecodeSetup(k.headers) for k in classes]
    yield v, ds, streams
    for d in ds:
        d.close()


@pytest.mark.parametrize("halfrate", [False, True], ids=["full", "half"])
def test_host_twin_equals_each_stream_alone(corpus, halfrate):
    v, ds, streams = corpus
    of = [c for c, _ in streams]
    assert len(set(of[:4])) == 4 and len(streams[7][1]) == 130 and streams[9][1] == []
    data, offs, gp, eo, first = R.csr(streams)
    status, begin, end, out_start, totals = v.decode_index_scan_host(ds, data, offs, gp, eo, stream_packets=first,
                                                                     halfrate=halfrate, classes=of)
    want = R.host_index(v, ds, streams, halfrate)
    for i, (st, b, e, o, t) in enumerate(want):
        a, z = int(first[i]), int(first[i + 1])
        assert np.array_equal(status[a:z], st) and np.array_equal(begin[a:z], b) and np.array_equal(end[a:z], e), i
        assert np.array_equal(out_start[a:z], o) and totals[i] == t, i
    assert totals[9] == 0 and (totals[:9] > 0).all()
    assert (status[int(first[10]):] != 0).sum() == 2                 # the truncated and the header packet
    # the classes matter: the same streams under one class give another index
    other = v.decode_index_scan_host(ds, data, offs, gp, eo, stream_packets=first, halfrate=halfrate,
                                     classes=[0] * len(of))
    assert not np.array_equal(other[4], totals)


def test_host_twin_argument_errors(corpus):
    v, ds, streams = corpus
    of = [c for c, _ in streams]
    data, offs, gp, eo, first = R.csr(streams)
    for bad in ([len(ds)] + of[1:], [-1] + of[1:]):
        with pytest.raises(v.VbmError, match=f"code {EINVAL}: .*class id"):
            v.decode_index_scan_host(ds, data, offs, gp, eo, stream_packets=first, classes=bad)
    with pytest.raises(ValueError, match="one class id per stream"):
        v.decode_index_scan_host(ds, data, offs, gp, eo, stream_packets=first, classes=of[1:])
    with pytest.raises(v.VbmError, match=f"code {EINVAL}"):
        v.decode_index_scan_host([], data, offs, gp, eo, stream_packets=first, classes=of)
    from vorbis_aotuv_lancer_amd._lib import lib
    none = [None] * 4 + [0] + [None] * 7                             # a rate that is neither 0 nor 1; no stream classes
    assert lib.vbm_host_decode_index_scan_mixed(1, None, 2, 1, *none) == EINVAL
    assert b"halfrate" in lib.vbm_last_error()
    assert lib.vbm_host_decode_index_scan_mixed(1, None, 0, 1, *none) == EINVAL


def ident(ch, e0, e1, rate=44100):
    """a Vorbis identification packet: the fields header_classes reads at their places"""
    return (b"\x01vorbis" + bytes(4) + bytes([ch]) + int(rate).to_bytes(4, "little") + bytes(12) +
            bytes([e1 << 4 | e0, 1]))


def test_header_grouping():
    from vorbis_aotuv_lancer_amd.decoder import header_classes
    a, b, c = ident(2, 8, 11), ident(1, 9, 9), ident(6, 8, 12)
    triples = [[a, b"comment 0", b"setup A"], [b, b"x", b"setup A"], [a, b"comment 2", b"setup A"],
               [a, b"x", b"setup B"], [c, b"x", b"setup C"], [b, b"y", b"setup A"]]
    ids, firsts, max_ch, max_bs = header_classes(triples)
    assert ids == [0, 1, 0, 2, 3, 1]                                  # by first appearance; the comments play no part
    assert firsts == [0, 1, 3, 4] and (max_ch, max_bs) == (6, 4096)
    assert header_classes(triples[:3]) == ([0, 1, 0], [0, 1], 2, 2048)
    assert header_classes(triples[1:2]) == ([0], [0], 1, 512)
    with pytest.raises(ValueError, match="identification"):
        header_classes([[b"\x01vorbi", b"", b""]])
