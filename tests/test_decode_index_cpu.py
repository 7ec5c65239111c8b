"""Host index of a stream's packets (vbm_decode_index, no GPU): per-packet status equals the host unpack's, and the
samples / out_start / total equal the tests' restatement of vorbis_synthesis_blockin's bookkeeping
(lib/block.c:1050-1161; blockin in tests/decode_packets.py), with trimmed starts, eos trims and failed packets."""
import ctypes as C

import numpy as np
import pytest

from tests.decode_packets import (DUMPS, EINVAL, INDEX_PACKS, csr, dump_packets, oracle_packets, pack_setup,
                                  page_granule_variants, restated, with_bad_packets)


def check_index(v, ds, packets, gps, eoss):
    data, offs = csr(packets)
    status, samples, out_start, total = v.decode_index(ds, data, offs, gps, eoss)
    want = restated(ds, packets, gps, eoss)
    assert list(status) == want[0]
    assert [ds.unpack(p)[0] for p in packets] == list(status)
    assert list(samples) == want[1]
    assert list(out_start) == want[2] and total == want[3]
    assert status.dtype == np.int32 and samples.dtype == np.int32 and out_start.dtype == np.int64
    return status, samples, out_start, total


@pytest.mark.parametrize("ch,rate,q,golden", DUMPS)
def test_index_of_the_reference_dumps(ch, rate, q, golden):
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(ch, rate, q))
    ds = v.DecodeSetup(h)
    packets = dump_packets(golden)
    for gps, eoss in page_granule_variants(ds, packets):
        check_index(v, ds, packets, gps, eoss)
    bad = with_bad_packets(packets, h, 5)
    status = check_index(v, ds, bad, [-1] * len(bad), [0] * len(bad))[0]
    assert sum(1 for s in status if s) >= 3          # two header packets, the empty one (others may parse)
    ds.close()


@pytest.mark.parametrize("pack", INDEX_PACKS)
def test_index_of_shipped_packs(oracle, pack):
    import vorbis_aotuv_lancer_amd as v
    setup, d = pack_setup(v, pack)
    h = v.header_packets(setup)
    ds = v.DecodeSetup(h)
    ch, rate = int(d["info/channels"][0]), int(d["info/rate"][0])
    q = float(d["info/quality"][0])
    packets = [b["packet"] for b in oracle_packets(oracle, ch, rate, q, seconds=2.0, seed=9)]
    for gps, eoss in page_granule_variants(ds, packets):
        check_index(v, ds, packets, gps, eoss)
    bad = with_bad_packets(packets, h, 6)
    for gps, eoss in page_granule_variants(ds, bad)[1:3]:
        check_index(v, ds, bad, gps, eoss)
    ds.close()


def test_index_clamps_offsets_and_handles_empty_streams():
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(2, 44100, 0.5))
    ds = v.DecodeSetup(h)
    packets = dump_packets("ref_scalar_2ch_44100_q05_20s.pkt")[:20]
    data, offs = csr(packets)
    status, samples, out_start, total = v.decode_index(ds, data, offs)
    # offsets past the data are clamped: the last packets become empty (VBM_ENOTAUDIO, as the device unpack says)
    cut = data[:int(offs[10])]
    st2, sm2, _, t2 = v.decode_index(ds, cut, offs)
    assert list(st2[:10]) == list(status[:10]) and all(s == -135 for s in st2[10:]) and t2 == sum(samples[:10])
    s0, n0, o0, t0 = v.decode_index(ds, np.zeros(0, np.uint8), np.zeros(1, np.int64))
    assert len(s0) == len(n0) == len(o0) == 0 and t0 == 0
    ds.close()


def test_index_bad_arguments():
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    ds = v.DecodeSetup(v.header_packets(v.Setup(2, 44100, 0.5)))
    data = np.zeros(8, np.uint8)
    offs = np.array([0, 4, 8], np.int64)
    out = [np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int64)]
    total = C.c_longlong()
    ptrs = [o.ctypes.data for o in out]
    assert lib.vbm_decode_index(None, 2, data.ctypes.data, offs.ctypes.data, 8, None, None, *ptrs, C.byref(total)) == EINVAL
    assert lib.vbm_decode_index(ds._h, -1, data.ctypes.data, offs.ctypes.data, 8, None, None, *ptrs, C.byref(total)) == EINVAL
    assert lib.vbm_decode_index(ds._h, 2, data.ctypes.data, None, 8, None, None, *ptrs, C.byref(total)) == EINVAL
    assert lib.vbm_decode_index(ds._h, 2, None, offs.ctypes.data, 8, None, None, *ptrs, C.byref(total)) == EINVAL
    assert lib.vbm_decode_index(ds._h, 2, data.ctypes.data, offs.ctypes.data, -1, None, None, *ptrs, C.byref(total)) == EINVAL
    assert lib.vbm_decode_index(ds._h, 2, data.ctypes.data, offs.ctypes.data, 8, None, None, None, ptrs[1], ptrs[2],
                                C.byref(total)) == EINVAL
    assert lib.vbm_decode_index(ds._h, 2, data.ctypes.data, offs.ctypes.data, 8, None, None, *ptrs, None) == EINVAL
    with pytest.raises(ValueError):
        v.decode_index(ds, data, offs, granulepos=np.zeros(3, np.int64))
    ds.close()


def test_index_of_a_long_stream_passes_2_to_the_31_samples():
    """a stream longer than 2^31 samples: out_start and total are 64-bit"""
    import vorbis_aotuv_lancer_amd as v
    ds = v.DecodeSetup(v.header_packets(v.Setup(2, 44100, 0.5)))
    packets = dump_packets("ref_scalar_2ch_44100_q05_20s.pkt")
    data, offs = csr(packets)
    _, samples, _, total = v.decode_index(ds, data, offs)
    reps = (2 ** 31) // total + 2
    n = len(packets)
    big_offs = np.concatenate([offs[:-1] + r * len(data) for r in range(reps)] + [offs[-1:] + (reps - 1) * len(data)])
    status, samples2, out_start, total2 = v.decode_index(ds, np.tile(data, reps), big_offs)
    assert total2 > 2 ** 31 and total2 == int(samples2.astype(np.int64).sum())
    assert out_start[-1] + samples2[-1] == total2 and np.all(np.diff(out_start) >= 0)
    assert list(samples2[:n]) == list(samples)
    ds.close()
