"""Range stores and the index built on the MI355X from a CSR in device memory (decode_index_device,
RangeStore.from_device, OggIndex(device_demux=True)): the device index equals its CPU twin and the serial host index
array for array, a store made on the device decodes every range to the bits of the host-made store, and an OggIndex
opened through the device demux equals the default one and decode_ogg."""
import ctypes

import numpy as np
import pytest
import torch

from tests.decode_calls import encoded, ranges, rows_tensor, runs_call, to_dev
from tests.decode_packets import BS, EINVAL, as_stream, join, one_byte_corpus, pack_setup, serial_index

GUARD = 64                                                 # canary elements on either side of every output
CANARY = {torch.int32: 0x5a5a5a5a, torch.int64: 0x5a5a5a5a5a5a5a5a}


def device_index(dec, data, offsets, gp, eos, first, cuda):
    """vbm_decode_index_device into buffers with canaries around them; the inputs must come back unchanged
    -> numpy (status, begin, end, out_start, totals)"""
    from vorbis_aotuv_lancer_amd._lib import lib
    first = np.ascontiguousarray(np.asarray(first, np.int64))
    P, S = len(offsets) - 1, len(first) - 1
    ins = [to_dev(x, cuda) for x in (data, offsets, gp, eos)]
    keep = [None if t is None else t.clone() for t in ins]
    outs = [torch.full((n + 2 * GUARD,), CANARY[dt], dtype=dt, device=cuda)
            for n, dt in ((P, torch.int32), (P, torch.int32), (P, torch.int32), (P, torch.int64), (S, torch.int64))]
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    rc = lib.vbm_decode_index_device(dec._h, S, first.ctypes.data, ptr(ins[0]), ins[1].data_ptr(), len(data), ptr(ins[2]),
                                     ptr(ins[3]), *[o.data_ptr() + GUARD * o.element_size() for o in outs],
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for t, k in zip(ins, keep):
        assert t is None or torch.equal(t, k), "an input was written"
    res = []
    for o in outs:
        h = o.cpu().numpy()
        assert np.all(h[:GUARD] == CANARY[o.dtype]) and np.all(h[len(h) - GUARD:] == CANARY[o.dtype]), "canary"
        res.append(h[GUARD:len(h) - GUARD])
    return res


def assert_device_index(v, ds, decs, data, offsets, gp, eos, first, cuda):
    """device == twin == serial host index, at the rate of every decoder of decs"""
    first = np.asarray(first, np.int64)
    for dec in decs:
        want = serial_index(v, ds, data, offsets, gp, eos, first, dec.halfrate)
        twin = v.decode_index_scan_host(ds, data, offsets, gp, eos, first, halfrate=dec.halfrate)
        got = device_index(dec, data, offsets, gp, eos, first, cuda)
        for g, t, name in zip(got, twin, ("status", "begin", "end", "out_start", "totals")):
            assert g.dtype == t.dtype and np.array_equal(g, t), f"{name}: device against its twin"
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2] - got[1], want[1])
        assert np.array_equal(got[3], want[2]) and np.array_equal(got[4], want[3])


@pytest.fixture(scope="module")
def world(cuda):
    """five short stereo streams (one with bursts, one with failed packets inserted), their setup and two decoders"""
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    h = v.header_packets(setup)
    pks = [encoded(v, setup, 1.0 + 0.25 * i, 300 + i, cuda, burst=i == 1) for i in range(5)]
    rng = np.random.default_rng(4)
    bad = list(pks[3])
    bad.insert(10, (h[2], -1, 0))
    bad.insert(20, (bad[19][0][:len(bad[19][0]) // 3], -1, 0))
    bad.insert(30, (rng.integers(0, 256, 200, dtype=np.uint8).tobytes(), -1, 0))
    for _ in range(5):
        bad.insert(41, (b"", -1, 0))
    bad.insert(0, (h[0], -1, 0))
    clean = list(pks)
    pks[3] = bad
    ds = v.DecodeSetup(h)
    assert tuple(ds.blocksizes) == BS
    w = dict(v=v, setup=setup, ds=ds, pks=pks, clean=clean, streams=[as_stream(pk) for pk in pks],
             dec=v.Decoder(ds, 2, 64), half=v.Decoder(ds, 1, 64, halfrate=True))
    yield w
    w["dec"].close()
    w["half"].close()
    ds.close()


# ---- the device index ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_index_of_one_byte_streams(cuda, world):
    v, ds = world["v"], world["ds"]
    streams = one_byte_corpus(seed=2, lengths=[0, 1, 63, 64, 65, 129, 200, 4097], shares=(0.0, 0.1, 0.9))
    data, offsets, gp, eos, first = join(streams)
    assert len(first) - 1 > 130
    assert_device_index(v, ds, [world["dec"], world["half"]], data, offsets, gp, eos, first, cuda)
    assert_device_index(v, ds, [world["dec"]], data, offsets, None, None, first, cuda)
    s = streams[-1]                                            # one stream alone, through the Python entry point
    got = v.decode_index_device(world["dec"], to_dev(s[0], cuda), to_dev(s[1], cuda), to_dev(s[2], cuda), to_dev(s[3], cuda))
    want = v.decode_index_scan_host(ds, *s)
    assert all(g.is_cuda and np.array_equal(g.cpu().numpy(), t) for g, t in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3, 65, 130])
def test_device_index_of_real_streams(cuda, world, S):
    v, ds = world["v"], world["ds"]
    order = [3, 1, 0, 2, 4]
    data, offsets, gp, eos, first = join([world["streams"][order[s % 5]] for s in range(S)])
    assert_device_index(v, ds, [world["dec"], world["half"]], data, offsets, gp, eos, first, cuda)


@pytest.mark.gpu
def test_more_streams_than_one_staging_slot_holds(cuda, world):
    """a decoder with a small staging slot (max_batch 2, one stream: 9 ints) takes the streams in several launches"""
    v, ds = world["v"], world["ds"]
    small = v.Decoder(ds, 1, 2)
    data, offsets, gp, eos, first = join([world["streams"][s % 5] for s in range(21)])
    assert_device_index(v, ds, [small], data, offsets, gp, eos, first, cuda)
    small.close()


@pytest.mark.gpu
def test_a_stream_whose_total_passes_2_to_the_31(cuda, world):
    v, ds = world["v"], world["ds"]
    P = 2 ** 21 + 8
    data = np.full(P, 2, np.uint8)                             # audio, mode 1 (long), lW = nW = 0
    offsets = np.arange(P + 1, dtype=np.int64)
    status, samples, out_start, total = v.decode_index(ds, data, offsets)
    assert total == 2147490816 and np.all(status == 0)
    got = device_index(world["dec"], data, offsets, None, None, [0, P], cuda)
    assert np.array_equal(got[0], status) and np.array_equal(got[2] - got[1], samples)
    assert np.array_equal(got[3], out_start) and int(got[4][0]) == total
    # granule positions beyond 2^31 and an eos trim at the end
    gp = np.full(P, -1, np.int64)
    gp[2 ** 21] = 2 ** 21 * 1024
    gp[-1] = (P - 1) * 1024 - 300
    eos = np.zeros(P, np.uint8)
    eos[-1] = 1
    assert_device_index(v, ds, [world["dec"]], data, offsets, gp, eos, [0, P], cuda)


# ---- stores ------------------------------------------------------------------------------------------------------
def range_set(ds, streams, seed, halfrate=False):
    """40 seeded ranges and the edge cases of test_edge_cases_and_overlapping_ranges, over all streams"""
    import vorbis_aotuv_lancer_amd as v
    idx = [v.decode_index(ds, *s, halfrate=halfrate) for s in streams]
    totals = [int(i[3]) for i in idx]
    rng = np.random.default_rng(seed)
    ids = [int(i) for i in rng.integers(0, len(streams), 40)]
    starts = [int(rng.integers(0, totals[i] + 10)) for i in ids]
    lengths = [int(rng.integers(0, 9000)) for _ in ids]
    for i, (_, samples, out_start, total) in enumerate(idx):
        e_starts = [0, 0, 5, total - 1, total - 100, total - 100, total, total + 50, 0]
        e_lengths = [1, 3000, 0, 1, 100, 5000, 10, 10, total if i == 0 else 4000]
        for k in range(3, len(samples), 9):                    # packet starts and +-1
            if samples[k]:
                for d in (-1, 0, 1):
                    e_starts.append(int(out_start[k]) + d)
                    e_lengths.append([1, 700, 2048][(k + d) % 3])
        e_starts = [max(s, 0) for s in e_starts]
        ids += [i] * len(e_starts)
        starts += e_starts
        lengths += e_lengths
    return ids, starts, lengths, totals


def device_store(v, dec, streams, cuda):
    data, offsets, gp, eos, first = join(streams)
    t = [to_dev(x, cuda) for x in (data, offsets, gp, eos)]
    return v.RangeStore.from_device(dec, *t, stream_packets=first), t


def assert_stores_equal(v, ds, streams, cuda, max_batch, halfrate=False, seed=7):
    dec = v.Decoder(ds, 1, max_batch, halfrate=halfrate)
    host = v.RangeStore(dec, streams)
    dev, tensors = device_store(v, dec, streams, cuda)
    ids, starts, lengths, totals = range_set(ds, streams, seed, halfrate)
    assert list(host.totals) == totals and np.array_equal(dev.totals, host.totals) and dev.halfrate == halfrate
    assert np.array_equal(dev.packets, host.packets)
    want = ranges(dec, host, ids, starts, lengths)
    got = ranges(dec, dev, ids, starts, lengths)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    assert sum(want[1]) > 0
    host.close()
    return dec, dev, tensors, (ids, starts, lengths), want


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch,halfrate", [(64, False), (7, False), (2, False), (64, True)])
def test_from_device_store_equals_the_host_store(cuda, world, max_batch, halfrate):
    v, ds = world["v"], world["ds"]
    dec, dev, _, _, _ = assert_stores_equal(v, ds, world["streams"], cuda, max_batch, halfrate)
    dev.close()
    dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pack", ["mode_1ch_8000_q0.5.vpk", "mode_6ch_48000_q0.5.vpk"])
def test_from_device_store_of_other_classes(cuda, pack):
    import vorbis_aotuv_lancer_amd as v
    setup, _ = pack_setup(v, pack)
    ds = v.DecodeSetup(v.header_packets(setup))
    if pack == "mode_1ch_8000_q0.5.vpk":
        assert ds.blocksizes == (512, 512)
    streams = [as_stream(encoded(v, setup, 1.0, 310, cuda, burst=True))]
    for halfrate in (False, True):
        dec, dev, _, _, _ = assert_stores_equal(v, ds, streams, cuda, 64, halfrate)
        dev.close()
        dec.close()
    ds.close()


@pytest.mark.gpu
def test_the_store_owns_its_bytes(cuda, world):
    v, ds = world["v"], world["ds"]
    dec, dev, tensors, rs, want = assert_stores_equal(v, ds, world["streams"], cuda, 64)
    tensors[0].fill_(0xa5)
    tensors[1].fill_(-(2 ** 40))
    tensors[2].fill_(-77)
    tensors[3].fill_(1)
    torch.cuda.synchronize()
    got = ranges(dec, dev, *rs)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    dev.close()
    dec.close()


# ---- OggIndex ------------------------------------------------------------------------------------------------------
def ogg_files(v, world, tmp_path):
    files = []
    for i, pk in enumerate(world["clean"]):
        blob = v.write_ogg(world["setup"], [p[0] for p in pk], [(p[1], p[2]) for p in pk], serialno=i)
        if i == 2:
            path = tmp_path / "two.ogg"
            path.write_bytes(blob)
            blob = str(path)
        files.append(blob)
    return files


@pytest.mark.gpu
def test_ogg_index_through_the_device_demux(cuda, world, tmp_path):
    v = world["v"]
    files = ogg_files(v, world, tmp_path)
    lin = [p.cpu().numpy() for p, _ in v.decode_ogg(files)]
    for halfrate in (False, True):
        host = v.OggIndex(files, max_batch=256, halfrate=halfrate)
        dev = v.OggIndex(files, max_batch=256, halfrate=halfrate, device_demux=True)
        assert np.array_equal(dev.total_samples, host.total_samples)
        assert (dev.channels, dev.rate, dev.halfrate) == (host.channels, host.rate, host.halfrate)
        rng = np.random.default_rng(12)
        ids = [int(i) for i in rng.integers(0, 5, 60)]
        starts = [int(rng.integers(0, host.total_samples[i])) for i in ids]
        lengths = [int(rng.integers(1, 20000)) for _ in ids]
        want, wgot = host.decode_ranges(ids, starts, lengths)
        pcm, got = dev.decode_ranges(ids, starts, lengths)
        pcm = pcm.cpu().numpy()
        assert np.array_equal(got, wgot) and np.array_equal(pcm, want.cpu().numpy())
        if not halfrate:
            assert list(dev.total_samples) == [x.shape[1] for x in lin]
            for r, (i, s, L) in enumerate(zip(ids, starts, lengths)):
                n = min(lin[i].shape[1] - s, L)
                assert got[r] == n and np.array_equal(pcm[r, :, :n], lin[i][:, s:s + n]) and np.all(pcm[r, :, n:] == 0)
        host.close()
        dev.close()


def first_page_len(blob):
    nseg = blob[26]
    return 27 + nseg + sum(blob[27:27 + nseg])


@pytest.mark.gpu
def test_ogg_index_device_demux_errors(cuda, world, tmp_path):
    v = world["v"]
    files = ogg_files(v, world, tmp_path)
    bad = bytearray(files[1])
    bad[first_page_len(files[1]) + 40] ^= 0x10                        # the "crc" corruption of test_ogg_demux_cpu.py
    with pytest.raises(v.VbmError, match="file 1"):
        v.OggIndex([files[0], bytes(bad), files[3]], device_demux=True)
    path = tmp_path / "broken.ogg"
    path.write_bytes(bytes(bad))
    with pytest.raises(v.VbmError, match="broken.ogg"):
        v.OggIndex([files[0], str(path)], device_demux=True)
    mono = v.Setup(1, 44100, 0.5)
    pk = encoded(v, mono, 0.5, 99, cuda)
    other = v.write_ogg(mono, [p[0] for p in pk], [(p[1], p[2]) for p in pk], serialno=9)
    with pytest.raises(ValueError, match="file 1 has other identification or setup headers"):
        v.OggIndex([files[0], other], device_demux=True)
    with pytest.raises(ValueError):
        v.OggIndex([], device_demux=True)


@pytest.mark.gpu
def test_from_device_takes_a_demux_batch(cuda, world, tmp_path):
    v, ds = world["v"], world["ds"]
    files = ogg_files(v, world, tmp_path)
    b = v.demux_ogg_device(files)
    assert not any(b.status)
    dec = v.Decoder(ds, 1, 64)
    dev = v.RangeStore.from_device(dec, b)
    host = v.RangeStore(dec, [v.demux_ogg(open(f, "rb").read() if isinstance(f, str) else f)[1:] for f in files])
    assert dev.nstreams == 5 and np.array_equal(dev.totals, host.totals)
    ids, starts, lengths = [0, 1, 2, 3, 4, 2], [0, 100, 5000, 20000, 77, 0], [3000, 1, 4096, 9000, 512, 0]
    want = ranges(dec, host, ids, starts, lengths)
    got = ranges(dec, dev, ids, starts, lengths)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
    dev.close()
    host.close()
    dec.close()


# ---- coexistence -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_stores_and_stream_calls_interleaved(cuda, world):
    """two device-made stores on one decoder; synthesis_runs, synthesis_batch and index calls between the range calls
    change nothing on either side"""
    v, ds, pks, streams = world["v"], world["ds"], world["pks"], world["streams"]
    lin_dec = v.Decoder(ds, 1, max(len(pk) for pk in pks))
    out = runs_call(lin_dec, [0], [pks[0]], cuda)
    lin0 = out[0][0, :, :int(out[1][0])].cpu().numpy()
    lin_dec.close()
    dec = world["dec"]                                                 # two streams, max_batch 64
    dec.reset()
    a, ta = device_store(v, dec, streams[:2], cuda)
    b, tb = device_store(v, dec, streams[2:], cuda)
    host_a, host_b = v.RangeStore(dec, streams[:2]), v.RangeStore(dec, streams[2:])
    parts = []
    pk = pks[0]
    for at in range(0, len(pk), 20):
        o = runs_call(dec, [1], [pk[at:at + 20]], cuda)
        parts.append(o[0][0, :, :int(o[1][0])].cpu().numpy())
        args_a = ([0, 1, 0], [at * 300, 1000 + at, 0], [2000, 17, 4000])
        args_b = ([2, 0, 1], [at * 200, 5 + at, 30000], [1500, 3000, 64])
        got_a, got_b = ranges(dec, a, *args_a), ranges(dec, b, *args_b)
        v.decode_index_device(dec, *tb, stream_packets=b.packets)     # an index call in between
        r, n = rows_tensor([pk[min(at, len(pk) - 1)][0]], cuda)
        dec.synthesis_batch([0], r, n)                                 # stream 0 stepwise, between range calls
        want_a, want_b = ranges(dec, host_a, *args_a), ranges(dec, host_b, *args_b)
        assert np.array_equal(got_a[1], want_a[1]) and np.array_equal(got_a[0], want_a[0])
        assert np.array_equal(got_b[1], want_b[1]) and np.array_equal(got_b[0], want_b[0])
    assert np.array_equal(np.concatenate(parts, axis=1), lin0)        # the runs of stream 1 saw none of it
    for s in (a, b, host_a, host_b):
        s.close()
    dec.reset()


@pytest.mark.gpu
def test_argument_errors_enqueue_nothing(cuda, world):
    v, ds = world["v"], world["ds"]
    from vorbis_aotuv_lancer_amd._lib import lib
    dec = world["dec"]
    data, offsets, gp, eos, first = join(world["streams"][:2])
    P = len(offsets) - 1
    t = [to_dev(x, cuda) for x in (data, offsets, gp, eos)]
    outs = [torch.full((P,), 77, dtype=dt, device=cuda) for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
    totals = torch.full((2,), 77, dtype=torch.int64, device=cuda)
    good = dict(dec=dec._h, S=2, first=first.ctypes.data, data=t[0].data_ptr(), offs=t[1].data_ptr(), nbytes=len(data),
                gp=t[2].data_ptr(), eos=t[3].data_ptr(), status=outs[0].data_ptr(), begin=outs[1].data_ptr(),
                end=outs[2].data_ptr(), out_start=outs[3].data_ptr(), totals=totals.data_ptr(), stream=None)
    nonzero = np.array([1, 5, P], np.int64)
    decreasing = np.array([0, P, P - 1], np.int64)
    huge = np.array([0, 5, 2 ** 31 - 1], np.int64)
    cases = [dict(dec=None), dict(S=0), dict(S=-1), dict(first=None), dict(nbytes=-1), dict(data=None), dict(offs=None),
             dict(first=nonzero.ctypes.data), dict(first=decreasing.ctypes.data), dict(first=huge.ctypes.data)]
    for kw in cases + [dict(status=None), dict(begin=None), dict(end=None), dict(out_start=None), dict(totals=None)]:
        assert lib.vbm_decode_index_device(*dict(good, **kw).values()) == EINVAL, kw
    h = ctypes.c_void_p()
    create = {k: good[k] for k in ("dec", "S", "first", "data", "offs", "nbytes", "gp", "eos", "stream")}
    for kw in cases:
        assert lib.vbm_range_store_create_device(ctypes.byref(h), *dict(create, **kw).values()) == EINVAL, kw
        assert not h.value
    assert lib.vbm_range_store_create_device(None, *create.values()) == EINVAL
    with pytest.raises(ValueError):
        v.RangeStore.from_device(dec, *t, stream_packets=[0, P - 1])
    with pytest.raises(ValueError):
        v.decode_index_device(dec, t[0], t[1], granulepos=t[2][:-1])
    torch.cuda.synchronize()
    assert all(torch.all(o == 77) for o in outs) and torch.all(totals == 77)
    # the refused calls left the decoder usable
    assert lib.vbm_decode_index_device(*good.values()) == 0
    torch.cuda.synchronize()
    want = v.decode_index_scan_host(ds, data, offsets, gp, eos, first)
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs + [totals], want))
    other = v.Decoder(ds, 1, 16)
    store, _ = device_store(v, dec, world["streams"][:1], cuda)
    with pytest.raises(v.VbmError, match=str(EINVAL)):
        other.synthesis_ranges(store, [0], [0], [100])                # a store of another decoder
    store.close()
    other.close()
