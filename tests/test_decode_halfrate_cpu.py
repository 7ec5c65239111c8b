"""Half-rate decoding, the host side (no GPU): vbm_decode_index_halfrate against the tests' restatement of
vorbis_synthesis_blockin's bookkeeping with halfrate_flag (reference lib/block.c:1050-1161; blockin in
tests/decode_packets.py), its halfrate = 0 form against vbm_decode_index, one derived stream length, and the argument
check of vbm_decoder_create_halfrate."""
import ctypes as C

import numpy as np
import pytest

from tests import vorbis_model as vm
from tests.decode_packets import EINVAL, ENODEV, csr, fromdB, random_stream_packets, restated, trim_granule_variants

PAIRS = [0, 3, 4, 5, 8, 14]            # vm.PAIRS: 256/256, 256/2048, 256/4096, 512/512, 512/4096, 4096/4096


def index(v, ds, packets, gps, eoss, halfrate):
    data, offs = csr(packets)
    return v.decode_index(ds, data, offs, gps, eoss, halfrate=halfrate)


@pytest.mark.parametrize("k", PAIRS, ids=[f"{vm.PAIRS[k][0]}_{vm.PAIRS[k][1]}" for k in PAIRS])
def test_index_equals_the_restatement_at_both_rates(k):
    import vorbis_aotuv_lancer_amd as v
    ds, packets = random_stream_packets(k, 500 + k)
    assert tuple(ds.blocksizes) == vm.PAIRS[k]
    trimmed = set()
    for name, gps, eoss in trim_granule_variants(ds, packets):
        full = None
        for hs in (0, 1):
            status, samples, out_start, total = index(v, ds, packets, gps, eoss, bool(hs))
            want = restated(ds, packets, gps, eoss, hs)
            assert np.array_equal(status, np.array(want[0], np.int32)), f"{name} hs={hs}: status"
            assert np.array_equal(samples, np.array(want[1], np.int32)), f"{name} hs={hs}: samples"
            assert np.array_equal(out_start, np.array(want[2], np.int64)), f"{name} hs={hs}: out_start"
            assert total == want[3], f"{name} hs={hs}: total"
            assert sum(1 for s in status if s) >= 3
            if hs == 0:
                full = samples
            elif not np.array_equal(2 * samples.astype(np.int64), full):
                trimmed.add(name)                            # an odd trim: the half-rate count is not half of it
    assert any(n.startswith("end trim") for n in trimmed) and any(n.startswith("start trim") for n in trimmed)
    ds.close()


@pytest.mark.parametrize("k", PAIRS[:3])
def test_halfrate_0_is_vbm_decode_index(k):
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    ds, packets = random_stream_packets(k, 600 + k)
    data, offs = csr(packets)
    P = len(packets)
    for name, gps, eoss in trim_granule_variants(ds, packets):
        gp, eo = np.array(gps, np.int64), np.array(eoss, np.uint8)
        a = [np.full(P, 77, np.int32), np.full(P, 77, np.int32), np.full(P, 77, np.int64)]
        b = [x.copy() for x in a]
        ta, tb = C.c_longlong(-5), C.c_longlong(-6)
        assert lib.vbm_decode_index(ds._h, P, data.ctypes.data, offs.ctypes.data, len(data), gp.ctypes.data,
                                    eo.ctypes.data, *[x.ctypes.data for x in a], C.byref(ta)) == 0
        assert lib.vbm_decode_index_halfrate(ds._h, 0, P, data.ctypes.data, offs.ctypes.data, len(data),
                                             gp.ctypes.data, eo.ctypes.data, *[x.ctypes.data for x in b],
                                             C.byref(tb)) == 0
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and ta.value == tb.value, name
        got = v.decode_index(ds, data, offs, gps, eoss)
        assert all(np.array_equal(x, y) for x, y in zip(a, got[:3])) and got[3] == ta.value
    total = C.c_longlong()
    out = [np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int64)]
    for bad in (2, -1):
        assert lib.vbm_decode_index_halfrate(ds._h, bad, P, data.ctypes.data, offs.ctypes.data, len(data), None, None,
                                             *[x.ctypes.data for x in out], C.byref(total)) == EINVAL
    ds.close()


@pytest.mark.parametrize("k", [0, 3, 7, 14])
def test_the_trim_is_halved_not_the_granule_position(k):
    """vm.pcm_streams ends each stream 37 samples short of its untrimmed full-rate length U.  Every blocksizes / 4 is
    even, so U / 2 is exact; the reference removes 37 >> 1 = 18 output samples (lib/block.c:1115): the half-rate
    length is U / 2 - 18, not (U - 37) >> 1 = U / 2 - 19."""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(k)
    ds = v.DecodeSetup(vm.pack_headers(setup, coding))
    model = vm.Model(setup, fromdB())
    for pk in vm.pcm_streams(model, 7000 + k):
        packets, gps, eoss = [p[0] for p in pk], [p[1] for p in pk], [p[2] for p in pk]
        U = gps[-1] + 37
        assert U % 2 == 0
        assert index(v, ds, packets, gps, eoss, False)[3] == U - 37
        assert index(v, ds, packets, gps, eoss, True)[3] == U // 2 - 18
    ds.close()


def test_create_halfrate_checks_its_flag_before_the_device():
    import torch
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    ds = v.DecodeSetup(v.header_packets(v.Setup(2, 44100, 0.5)))
    for bad in (2, -1, 256):
        h = C.c_void_p()
        assert lib.vbm_decoder_create_halfrate(C.byref(h), ds._h, 1, 1, bad) == EINVAL
        assert not h.value
    if not torch.cuda.is_available():
        for flag in (0, 1):
            h = C.c_void_p()
            assert lib.vbm_decoder_create_halfrate(C.byref(h), ds._h, 1, 1, flag) == ENODEV
    assert lib.vbm_decoder_halfrate(None) == EINVAL
    ds.close()


def test_output_rate():
    from vorbis_aotuv_lancer_amd.decoder import output_rate
    assert output_rate(44100, False) == 44100 and output_rate(44100, True) == 22050
    assert isinstance(output_rate(44100, True), int)
    assert output_rate(11025, True) == 5512.5 and isinstance(output_rate(11025, True), float)
