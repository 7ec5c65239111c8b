"""The chunked index scan on the CPU (vbm_host_decode_index_scan: the code of the device kernel k_index_scan, its 64
lanes as a loop; no GPU) equals the serial host index (vbm_decode_index_halfrate) of each stream alone, array for
array, at both rates: on the corpora of test_decode_index_cpu.py, on seeded streams of one-byte packets with
adversarial granule positions and eos flags (the granulepos values below -1 included, which send a stream down the
serial fallback), and on CSRs with empty streams and offsets that are negative, past the data or decreasing."""
import ctypes as C

import numpy as np
import pytest

from tests.decode_packets import (BS, DUMPS, EINVAL, GP_KINDS, INDEX_PACKS, csr, dump_packets, join, one_byte_corpus,
                                  one_byte_stream, oracle_packets, pack_setup, page_granule_variants, serial_index,
                                  with_bad_packets)


def assert_scan_equals_serial(v, ds, data, offsets, gp, eos, first):
    """-> the twin's outputs at full rate"""
    first = np.asarray(first, np.int64)
    full = None
    for halfrate in (False, True):
        want = serial_index(v, ds, data, offsets, gp, eos, first, halfrate)
        status, begin, end, out_start, totals = v.decode_index_scan_host(ds, data, offsets, gp, eos, first,
                                                                         halfrate=halfrate)
        assert status.dtype == np.int32 and begin.dtype == np.int32 and out_start.dtype == np.int64
        assert np.array_equal(status, want[0])
        assert np.array_equal(end - begin, want[1])
        assert np.array_equal(out_start, want[2])
        assert np.array_equal(totals, want[3])
        assert np.all(begin >= 0) and np.all(begin[status != 0] == 0) and np.all(end[status != 0] == 0)
        full = full or (status, begin, end, out_start, totals)
    return full


@pytest.fixture(scope="module")
def ds2():
    import vorbis_aotuv_lancer_amd as v
    ds = v.DecodeSetup(v.header_packets(v.Setup(2, 44100, 0.5)))
    assert tuple(ds.blocksizes) == BS and ds.modes == 2
    yield ds
    ds.close()


def test_one_byte_streams_every_length_share_and_granule_kind(ds2):
    import vorbis_aotuv_lancer_amd as v
    streams = one_byte_corpus()
    seen_fallback = seen_scan = 0
    for s in streams:                                                  # each stream alone
        status = assert_scan_equals_serial(v, ds2, s[0], s[1], s[2], s[3], [0, len(s[2])])[0]
        below = bool(np.any((status == 0) & (s[2] < -1)))
        seen_fallback += below
        seen_scan += not below and len(s[2]) > 64 and bool(np.any(s[2] != -1))
    assert seen_fallback > 20 and seen_scan > 20                       # both paths are exercised, past one chunk
    data, offsets, gp, eos, first = join(streams)                      # all of them as streams of one CSR
    assert_scan_equals_serial(v, ds2, data, offsets, gp, eos, first)


def test_granule_kinds_trim_and_the_fallback_values_matter(ds2):
    """the corpus is adversarial: granule positions change sample counts, at starts and at eos"""
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(3)
    changed = 0
    for kind in GP_KINDS[1:]:
        data, o, gp, eos = one_byte_stream(rng, 200, 0.1, kind, 1)
        with_gp = v.decode_index_scan_host(ds2, data, o, gp, eos)
        without = v.decode_index_scan_host(ds2, data, o, None, None)
        changed += not np.array_equal(with_gp[2] - with_gp[1], without[2] - without[1])
    assert changed >= 5


# ---- the corpora of test_decode_index_cpu.py -----------------------------------------------------------------------
def real_streams(ds, packets, headers, seed):
    """every granule variant of the packets, and of the packets with failed ones inserted"""
    out = []
    for pk in (packets, with_bad_packets(packets, headers, seed)):
        data, offs = csr(pk)
        for gps, eoss in page_granule_variants(ds, pk):
            out.append((data, offs, np.asarray(gps, np.int64), np.asarray(eoss, np.uint8)))
    return out


def check_real(v, ds, streams):
    for s in streams:
        status = assert_scan_equals_serial(v, ds, s[0], s[1], s[2], s[3], [0, len(s[2])])[0]
    assert np.any(status != 0)                                         # the last one holds failed packets
    assert_scan_equals_serial(v, ds, *join(streams))


@pytest.mark.parametrize("ch,rate,q,golden", DUMPS)
def test_reference_dumps(ch, rate, q, golden):
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(ch, rate, q))
    ds = v.DecodeSetup(h)
    packets = dump_packets(golden)
    check_real(v, ds, real_streams(ds, packets, h, 5))
    ds.close()


@pytest.mark.parametrize("pack", INDEX_PACKS)
def test_shipped_packs(oracle, pack):
    import vorbis_aotuv_lancer_amd as v
    setup, d = pack_setup(v, pack)
    h = v.header_packets(setup)
    ds = v.DecodeSetup(h)
    ch, rate, q = int(d["info/channels"][0]), int(d["info/rate"][0]), float(d["info/quality"][0])
    packets = [b["packet"] for b in oracle_packets(oracle, ch, rate, q, seconds=2.0, seed=9)]
    check_real(v, ds, real_streams(ds, packets, h, 6))
    ds.close()


# ---- further CSR cases -------------------------------------------------------------------------------------------
def test_empty_streams_between_full_ones_and_null_granulepos_and_eos(ds2):
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(11)
    empty = one_byte_stream(rng, 0, 0.0, "none", 0)
    full = [one_byte_stream(rng, n, 0.1, "jitter0", 1) for n in (70, 1, 129)]
    data, offsets, gp, eos, first = join([empty, full[0], empty, empty, full[1], full[2], empty])
    assert list(np.diff(first)) == [0, 70, 0, 0, 1, 129, 0]
    totals = assert_scan_equals_serial(v, ds2, data, offsets, gp, eos, first)[4]
    assert list(totals[[0, 2, 3, 6]]) == [0, 0, 0, 0] and totals[1] > 0 and totals[5] > 0
    for g, e in ((None, eos), (gp, None), (None, None)):
        assert_scan_equals_serial(v, ds2, data, offsets, g, e, first)
    # only empty streams, and no data at all
    t = assert_scan_equals_serial(v, ds2, np.zeros(0, np.uint8), np.zeros(1, np.int64), None, None, [0, 0, 0])[4]
    assert list(t) == [0, 0]


def test_offsets_negative_past_the_data_and_decreasing():
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(2, 44100, 0.5))
    ds = v.DecodeSetup(h)
    packets = dump_packets("ref_scalar_2ch_44100_q05_20s.pkt")[:150]
    data, offs = csr(packets)
    first = [0, 40, 40, 110, 150]
    rng = np.random.default_rng(2)
    wild = offs.copy()
    wild[3] = -5
    wild[20:23] = [-(2 ** 40), -1, -7]
    wild[60:64] = wild[60:64][::-1]                     # decreasing
    wild[100] = wild[90]
    wild[130:] += len(data)                             # past the data
    wild[149] = 2 ** 62
    st = assert_scan_equals_serial(v, ds, data, wild, None, None, first)[0]
    assert np.any(st != 0) and np.any(st == 0)
    cut = data[:int(offs[75])]                          # data shorter than the offsets say
    st = assert_scan_equals_serial(v, ds, cut, offs, None, None, first)[0]
    assert np.all(st[76:] == -135) and np.all(st[:75] == 0)
    noise = rng.integers(-50, len(data) + 50, len(offs)).astype(np.int64)
    assert_scan_equals_serial(v, ds, data, noise, None, None, first)
    ds.close()


def test_bad_arguments(ds2):
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    data = np.zeros(8, np.uint8)
    offs = np.array([0, 4, 8], np.int64)
    first = np.array([0, 1, 2], np.int64)
    outs = [np.full(2, 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.int64),
            np.full(2, 77, np.int64)]
    good = dict(ds=ds2._h, halfrate=0, nstreams=2, first=first.ctypes.data, data=data.ctypes.data,
                offs=offs.ctypes.data, nbytes=8, gp=None, eos=None, status=outs[0].ctypes.data,
                begin=outs[1].ctypes.data, end=outs[2].ctypes.data, out_start=outs[3].ctypes.data,
                totals=outs[4].ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return lib.vbm_host_decode_index_scan(*a.values())

    dec = np.array([0, 2, 1], np.int64)
    nonzero = np.array([1, 1, 2], np.int64)
    huge = np.array([0, 1, 2 ** 31 - 1], np.int64)
    for kw in (dict(ds=None), dict(halfrate=2), dict(halfrate=-1), dict(nstreams=0), dict(nstreams=-3), dict(first=None),
               dict(nbytes=-1), dict(data=None), dict(offs=None), dict(totals=None), dict(status=None),
               dict(begin=None), dict(end=None), dict(out_start=None), dict(first=dec.ctypes.data),
               dict(first=nonzero.ctypes.data), dict(first=huge.ctypes.data)):
        assert call(**kw) == EINVAL, kw
        assert all(np.all(o == 77) for o in outs), kw                   # nothing is written on an error
    assert call() == 0
    assert call(data=None, nbytes=0) == 0                               # no data: every packet is empty
    assert list(outs[0]) == [-135, -135]
    with pytest.raises(ValueError):
        v.decode_index_scan_host(ds2, data, offs, granulepos=np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        v.decode_index_scan_host(ds2, data, offs, stream_packets=[0, 1])


def test_the_device_entry_points_are_exported():
    from vorbis_aotuv_lancer_amd._lib import lib
    assert lib.vbm_decode_index_device(None, 1, None, None, None, 0, None, None, None, None, None, None, None,
                                       None) == EINVAL
    h = C.c_void_p()
    assert lib.vbm_range_store_create_device(C.byref(h), None, 1, None, None, None, 0, None, None, None) == EINVAL
    assert not h.value
