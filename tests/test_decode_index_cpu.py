"""Host index of a stream's packets (vbm_decode_index, no GPU): per-packet status equals the host unpack's, and the
samples / out_start / total equal a Python restatement of vorbis_synthesis_blockin's bookkeeping
(lib/block.c:1050-1161), with trimmed starts, eos trims and failed packets."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_decoder_cpu import oracle_packets, pack_setup

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EINVAL = -131


def split_dump(d):
    out, at = [], 0
    while at < len(d):
        n = int.from_bytes(d[at:at + 4], "little")
        out.append(d[at + 4:at + 4 + n])
        at += 4 + n
    return out


def csr(packets):
    data = np.frombuffer(b"".join(packets), np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in packets]).astype(np.int64)
    return data, offs


def restated(ds, packets, gps, eoss):
    """lib/block.c:1050-1161 in Python over the host unpack's status and W -> (status, samples, out_start, total)"""
    bs = ds.blocksizes
    lW, sc, gp, at = -1, -1, -1, 0
    status, samples, out_start = [], [], []
    for p, vgp, eof in zip(packets, gps, eoss):
        rc, info = ds.unpack(p)[:2]
        status.append(rc)
        out_start.append(at)
        if rc:
            samples.append(0)
            continue
        W = info[1]
        begin, end = 0, 0
        if lW >= 0:
            end = bs[lW] // 4 + bs[W] // 4
        step = (bs[lW] // 4 if lW >= 0 else 0) + bs[W] // 4
        sc = 0 if sc == -1 else sc + step
        if gp == -1:
            if vgp != -1:
                gp = vgp
                if sc > gp:
                    extra = max(sc - vgp, 0)
                    if eof:
                        extra = min(extra, end - begin)
                        end -= extra
                    else:
                        begin = min(begin + extra, end)
        else:
            gp += step
            if vgp != -1 and gp != vgp:
                if gp > vgp:
                    extra = gp - vgp
                    if extra and eof:
                        extra = max(min(extra, end - begin), 0)
                        end -= extra
                gp = vgp
        samples.append(end - begin)
        at += end - begin
        lW = W
    return status, samples, out_start, at


def true_granules(ds, packets):
    """the granulepos an encoder writes after each packet (sum of the blockin steps; 0 for failed packets' slots)"""
    bs, lW, g, out = ds.blocksizes, -1, 0, []
    for p in packets:
        rc, info = ds.unpack(p)[:2]
        if rc == 0:
            if lW >= 0:
                g += bs[lW] // 4 + bs[info[1]] // 4
            lW = info[1]
        out.append(g)
    return out


def with_bad_packets(packets, headers, seed):
    rng = np.random.default_rng(seed)
    bad = list(packets)
    bad.insert(min(10, len(bad)), headers[2])
    bad.insert(min(20, len(bad)), packets[min(19, len(packets) - 1)][:len(packets[min(19, len(packets) - 1)]) // 3])
    bad.insert(min(30, len(bad)), rng.integers(0, 256, 200, dtype=np.uint8).tobytes())
    bad.insert(min(31, len(bad)), b"")
    bad.insert(0, headers[0])
    bad.insert(1, b"\x00")                               # a one-byte audio packet: the mode is missing
    return bad


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


def granule_variants(ds, packets):
    """(granulepos, eos) lists: none; on every 7th packet and the last with eos; a lowered first granulepos
    (trimmed start); an eos trim of 300 samples"""
    n, g = len(packets), true_granules(ds, packets)
    none = ([-1] * n, [0] * n)
    pages = ([g[k] if (k % 7 == 6 or k == n - 1) else -1 for k in range(n)], [0] * (n - 1) + [1])
    low = list(pages[0])
    first = next(k for k in range(n) if low[k] != -1)
    low[first] = max(low[first] - 700, 0)
    trim = list(pages[0])
    trim[-1] = max(trim[-1] - 300, 0)
    return [none, pages, (low, pages[1]), (trim, pages[1])]


@pytest.mark.parametrize("ch,rate,q,golden", [
    (2, 44100, 0.5, "ref_scalar_2ch_44100_q05_20s.pkt"),
    (6, 48000, 0.8, "ref_scalar_6ch_48000_q08_10s.pkt"),
])
def test_index_of_the_reference_dumps(ch, rate, q, golden):
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(ch, rate, q))
    ds = v.DecodeSetup(h)
    packets = split_dump(open(os.path.join(G, golden), "rb").read())
    for gps, eoss in granule_variants(ds, packets):
        check_index(v, ds, packets, gps, eoss)
    bad = with_bad_packets(packets, h, 5)
    status = check_index(v, ds, bad, [-1] * len(bad), [0] * len(bad))[0]
    assert sum(1 for s in status if s) >= 3          # two header packets, the empty one (others may parse)
    ds.close()


@pytest.mark.parametrize("pack", ["mode_1ch_44100_q0.5.vpk", "mode_2ch_44100_q0.1.vpk", "mode_2ch_96000_q0.5.vpk",
                                  "mode_1ch_8000_q0.5.vpk", "mode_6ch_48000_q0.5.vpk", "mode_2ch_44100_q-0.1.vpk"])
def test_index_of_shipped_packs(oracle, pack):
    import vorbis_aotuv_lancer_amd as v
    setup, d = pack_setup(v, pack)
    h = v.header_packets(setup)
    ds = v.DecodeSetup(h)
    ch, rate = int(d["info/channels"][0]), int(d["info/rate"][0])
    q = float(d["info/quality"][0])
    packets = [b["packet"] for b in oracle_packets(oracle, ch, rate, q, seconds=2.0, seed=9)]
    for gps, eoss in granule_variants(ds, packets):
        check_index(v, ds, packets, gps, eoss)
    bad = with_bad_packets(packets, h, 6)
    for gps, eoss in granule_variants(ds, bad)[1:3]:
        check_index(v, ds, bad, gps, eoss)
    ds.close()


def test_index_clamps_offsets_and_handles_empty_streams():
    import vorbis_aotuv_lancer_amd as v
    h = v.header_packets(v.Setup(2, 44100, 0.5))
    ds = v.DecodeSetup(h)
    packets = split_dump(open(os.path.join(G, "ref_scalar_2ch_44100_q05_20s.pkt"), "rb").read())[:20]
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
    packets = split_dump(open(os.path.join(G, "ref_scalar_2ch_44100_q05_20s.pkt"), "rb").read())
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
