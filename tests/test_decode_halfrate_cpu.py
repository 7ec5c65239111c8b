"""Half-rate decoding, the host side (no GPU): vbm_decode_index_halfrate against a Python restatement of
vorbis_synthesis_blockin's bookkeeping with halfrate_flag (reference lib/block.c:1050-1161), its halfrate = 0 form
against vbm_decode_index, one derived stream length, and the argument check of vbm_decoder_create_halfrate."""
import ctypes as C

import numpy as np
import pytest

from tests import vorbis_model as vm
from tests.test_decoder_model_cpu import fromdB

EINVAL, ENODEV = -131, -1000
PAIRS = [0, 3, 4, 5, 8, 14]            # vm.PAIRS: 256/256, 256/2048, 256/4096, 512/512, 512/4096, 4096/4096


def csr(packets):
    data = np.frombuffer(b"".join(packets), np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in packets]).astype(np.int64)
    return data, offs


def restated(ds, packets, gps, eoss, hs):
    """lib/block.c:1050-1161 with hs = ci->halfrate_flag, over the host unpack's status and W.  pcm_returned and
    pcm_current are taken relative to the packet's first final sample -> (status, samples, out_start, total)"""
    bs = ds.blocksizes
    lW, sample_count, granulepos, at = -1, -1, -1, 0
    status, samples, out_start = [], [], []
    for p, vb_granulepos, eofflag in zip(packets, gps, eoss):
        rc, info = ds.unpack(p)[:2]
        status.append(rc)
        out_start.append(at)
        if rc:
            samples.append(0)
            continue
        W = info[1]
        if lW < 0:                                           # pcm_returned == -1: both at thisCenter
            pcm_returned = pcm_current = 0
        else:                                                # :1059-1062
            pcm_returned = 0
            pcm_current = (bs[lW] // 4 + bs[W] // 4) >> hs
        if sample_count == -1:                               # :1078-1082
            sample_count = 0
        else:
            sample_count += bs[lW] // 4 + bs[W] // 4
        if granulepos == -1:                                 # :1084-1125
            if vb_granulepos != -1:
                granulepos = vb_granulepos
                if sample_count > granulepos:
                    extra = sample_count - vb_granulepos
                    if extra < 0:
                        extra = 0
                    if eofflag:
                        if extra > (pcm_current - pcm_returned) << hs:
                            extra = (pcm_current - pcm_returned) << hs
                        pcm_current -= extra >> hs
                    else:
                        pcm_returned += extra >> hs
                        if pcm_returned > pcm_current:
                            pcm_returned = pcm_current
        else:                                                # :1126-1157
            granulepos += bs[lW] // 4 + bs[W] // 4
            if vb_granulepos != -1 and granulepos != vb_granulepos:
                if granulepos > vb_granulepos:
                    extra = granulepos - vb_granulepos
                    if extra:
                        if eofflag:
                            if extra > (pcm_current - pcm_returned) << hs:
                                extra = (pcm_current - pcm_returned) << hs
                            if extra < 0:
                                extra = 0
                            pcm_current -= extra >> hs
                granulepos = vb_granulepos
        n = pcm_current - pcm_returned                       # vorbis_synthesis_pcmout + _read
        samples.append(n)
        at += n
        lW = W
    return status, samples, out_start, at


def stream_packets(k, seed):
    """a seeded random stream on block-size pair k: 40 packets whose W sequence has all four transitions (when the
    pair has two sizes), with failed packets inside -> (ds, packets)"""
    import vorbis_aotuv_lancer_amd as v
    setup, coding = vm.pcm_setup(k)
    h = vm.pack_headers(setup, coding)
    ds = v.DecodeSetup(h)
    model = vm.Model(setup, fromdB())
    rng = np.random.default_rng(seed)
    seq = "SSLLS" + "".join(rng.choice(["S", "L"], 35))
    packets = [p for p, _, _ in vm.pcm_streams(model, seed, sequences=[seq])[0]]
    W = [ds.unpack(p)[1][1] for p in packets]
    if ds.blocksizes[0] != ds.blocksizes[1]:
        assert {(a, b) for a, b in zip(W, W[1:])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    modes, bits = len(setup["modes"]), model.modebits
    packets.insert(9, h[2])                                  # a header packet: VBM_ENOTAUDIO
    packets.insert(17, b"")                                  # the empty packet
    if modes < (1 << bits):
        w = vm.BitWriter()
        w.write(0, 1)
        w.write(modes, bits)                                 # a mode past the last: VBM_EBADPACKET
        w.write(0xABCDE, 20)
        packets.insert(23, w.tobytes())
    packets.insert(1, h[0])                                  # a failed packet before the second block
    return ds, packets


def true_granules(ds, packets):
    """the granule position after each packet, in full-rate samples (failed packets repeat the last)"""
    bs, lW, g, out = ds.blocksizes, -1, 0, []
    for p in packets:
        rc, info = ds.unpack(p)[:2]
        if rc == 0:
            if lW >= 0:
                g += bs[lW] // 4 + bs[info[1]] // 4
            lW = info[1]
        out.append(g)
    return out


def granule_variants(ds, packets):
    """(name, granulepos, eos): absent; exact; the last packet short by odd and even amounts (end trim), with and
    without earlier positions; the first marked packet short by odd and even amounts (start trim), and by more than
    it returns; the last packet backdated by more than the stream holds (the clamp), with and without earlier
    positions; a start trim on the stream's first packet"""
    n, g = len(packets), true_granules(ds, packets)
    valid = [k for k in range(n) if ds.unpack(packets[k])[0] == 0]
    assert valid[-1] == n - 1
    eos = [0] * (n - 1) + [1]
    exact = [g[k] if (k in valid and (k % 5 == 4 or k == n - 1)) else -1 for k in range(n)]
    first = next(k for k in range(n) if exact[k] != -1)
    out = [("absent", [-1] * n, [0] * n), ("exact", exact, eos)]
    for d in (1, 2, 37, 300, 301):
        a = list(exact)
        a[-1] = g[-1] - d
        out.append((f"end trim {d}", a, eos))
        b = [-1] * (n - 1) + [g[-1] - d]                     # the first marked packet is the last: lib/block.c:1102
        out.append((f"end trim {d}, no earlier position", b, eos))
        c = list(exact)
        c[first] = g[first] - d
        out.append((f"start trim {d}", c, eos))
    c = list(exact)
    c[first] = max(g[first] - 3 * ds.blocksizes[1], 0)
    out.append(("start trim past the packet", c, eos))
    a = list(exact)
    a[-1] = 0
    out.append(("backdated last packet", a, eos))
    out.append(("backdated last packet, no earlier position", [-1] * (n - 1) + [0], eos))
    odd = list(exact)
    odd[-1] = 1
    out.append(("backdated to 1", odd, eos))
    z = list(exact)
    z[0] = 0                                                 # sample_count 0 is not past 0: nothing trimmed
    out.append(("position on the first packet", z, eos))
    return out


def index(v, ds, packets, gps, eoss, halfrate):
    data, offs = csr(packets)
    return v.decode_index(ds, data, offs, gps, eoss, halfrate=halfrate)


@pytest.mark.parametrize("k", PAIRS, ids=[f"{vm.PAIRS[k][0]}_{vm.PAIRS[k][1]}" for k in PAIRS])
def test_index_equals_the_restatement_at_both_rates(k):
    import vorbis_aotuv_lancer_amd as v
    ds, packets = stream_packets(k, 500 + k)
    assert tuple(ds.blocksizes) == vm.PAIRS[k]
    trimmed = set()
    for name, gps, eoss in granule_variants(ds, packets):
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
    ds, packets = stream_packets(k, 600 + k)
    data, offs = csr(packets)
    P = len(packets)
    for name, gps, eoss in granule_variants(ds, packets):
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
