"""The live range store on the MI355X (LiveRangeStore: vbm_live_store_*, csrc/live_store.hip): the device store against
its host twin append by append, sample windows of a store fed from an OggFeed against the linear decode of the same
results (with and without trims, at full and half rate, with gap marks, over two classes of a MixedDecoder), and cuts of
a live store against their own decode and against the host cutter over a snapshot."""
import numpy as np
import pytest
import torch

import vorbis_aotuv_lancer_amd as v
from tests import ogg_pages
from tests.decode_calls import FILL_RANGES, check, encoded, linear, ranges, to_dev
from tests.decode_packets import EINVAL, headers_of, one_byte_stream
from tests.live_store_cases import padded
from vorbis_aotuv_lancer_amd.decoder import LIVE_EBIG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def material(cuda):
    """three 1.5 s stereo q5 files from the product's encoder: (setup, DecodeSetup, per file its packets, the files)"""
    setup = v.Setup(2, 44100, 0.5)
    ds = v.DecodeSetup(v.header_packets(setup))
    pks = [encoded(v, setup, 1.5, 40 + i, cuda, burst=i == 1) for i in range(3)]
    files = [v.write_ogg(setup, [p[0] for p in pk], [(p[1], p[2]) for p in pk], serialno=90 + i)
             for i, pk in enumerate(pks)]
    yield setup, ds, pks, files
    ds.close()


def append_result(store, r, cap, gap=None):
    """a FeedResult into the store: all entries in one call, zero counts included; an entry of more than cap packets in
    calls of at most cap, its packets' offsets a slice of the result's"""
    if int(r.counts.max(initial=0)) <= cap:
        out = store.append(r.ids, r.counts, r.payload, r.offsets, granulepos=r.granulepos, eos=r.eos, gap=gap)
        assert not out.status.any()
        return
    a = 0
    for sid, c in zip(r.ids.tolist(), r.counts.tolist()):
        for b in range(a, a + c, cap):
            k = min(cap, a + c - b)
            out = store.append([sid], [k], r.payload, r.offsets[b:b + k + 1], granulepos=r.granulepos[b:b + k],
                               eos=r.eos[b:b + k], gap=None if gap is None else gap[b:b + k])
            assert not out.status.any()
        a += c


class Linear:
    """per slot the PCM synthesis_runs returned so far"""

    def __init__(self, S):
        self.parts, self.cat = [[] for _ in range(S)], [None] * S

    def add(self, ids, pcm, n):
        n = n.cpu().tolist()
        for row, sid in enumerate(ids):
            self.parts[sid].append(pcm[row, :, :n[row]].cpu().numpy())
            self.cat[sid] = None

    def of(self, sid, channels):
        if self.cat[sid] is None:
            self.cat[sid] = (np.concatenate(self.parts[sid], axis=1) if self.parts[sid]
                             else np.zeros((channels, 0), np.float32))
        return self.cat[sid]


def check_windows(dec, store, lin, rng, slots, channels=None):
    """seeded windows of the slots in [first_sample, totals) against the slices of lin, and one in front of each
    first_sample"""
    ids, starts, lengths, early = [], [], [], []
    for sid in slots:
        lo, T = int(store.first_sample[sid]), int(store.totals[sid])
        assert lin.of(sid, dec.channels).shape[1] == T
        if lo > 0:
            early.append((sid, lo - 1))
        if T == lo:
            continue
        w = [(lo, 1), (lo, min(T - lo, 3000)), (max(lo, T - 700), T - max(lo, T - 700)), (max(lo, T - 50), 400), (T - 1, 1)]
        for _ in range(3):
            s0 = int(rng.integers(lo, T))
            w.append((s0, int(rng.integers(1, 2500))))
        for s0, L in w:
            ids.append(sid), starts.append(s0), lengths.append(L)
    if ids:
        pcm, got = ranges(dec, store, ids, starts, lengths)
        if channels is None:
            check({s: lin.of(s, dec.channels) for s in slots}, ids, starts, lengths, pcm, got, "live")
        else:                                               # a mixed decoder: each range in its slot's channels
            for r, (sid, s0, L) in enumerate(zip(ids, starts, lengths)):
                want = lin.of(sid, channels[sid])[:, s0:s0 + L]
                assert got[r] == want.shape[1] and np.array_equal(pcm[r, :channels[sid], :got[r]], want), f"range {r}"
                assert np.all(pcm[r, channels[sid]:] == FILL_RANGES) and np.all(pcm[r, :, got[r]:] == FILL_RANGES)
    if early:
        pcm, got = ranges(dec, store, [e[0] for e in early], [e[1] for e in early], [10] * len(early))
        assert not got.any() and np.all(pcm == FILL_RANGES), "a window in front of first_sample"
    return len(ids), len(early)


# ---- 1. the device store against the twin --------------------------------------------------------------------------
def test_device_equals_twin(cuda):
    ds = v.DecodeSetup(headers_of(2, 44100, 0.5))
    dec = v.Decoder(ds, 1, 64)
    rng = np.random.default_rng(11)
    S, MP, MB = 5, 8, 200
    dev, twin = v.LiveRangeStore(dec, S, MP, MB), v.LiveRangeStore(ds, S, MP, MB, host=True)
    streams = {s: padded(one_byte_stream(rng, 400, inv, kind, 1), rng, 40)
               for s, inv, kind in ((0, 0.0, "jitter"), (1, 0.1, "minus2"), (2, 0.9, "none"), (4, 0.1, "big"))}
    at = dict.fromkeys(streams, 0)
    big = 0
    for step in range(40):
        if step == 20:
            dev.restart([4]), twin.restart([4])
        ids = [s for s in streams if rng.random() < 0.7]
        counts = [int(rng.integers(0, 11)) for _ in ids]             # up to 10: above the 8 slots now and then
        parts, sizes, gp, eos, gap = [], [], [], [], []
        for s, c in zip(ids, counts):
            data, off, g, e = streams[s]
            a = at[s]
            parts.append(data[off[a]:off[a + c]]), sizes.append(np.diff(off[a:a + c + 1]))
            gp.append(g[a:a + c]), eos.append(e[a:a + c]), gap.append((rng.random(c) < 0.1).astype(np.uint8))
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)      # noqa: E731
        data, gp, eos, gap = cat(parts, np.uint8), cat(gp, np.int64), cat(eos, np.uint8), cat(gap, np.uint8)
        offs = np.concatenate([[0], np.cumsum(cat(sizes, np.int64))]).astype(np.int64)
        rt = twin.append(ids, counts, data, offs, gp, eos, gap)
        rd = dev.append(ids, counts, *(to_dev(x, cuda) for x in (data, offs, gp, eos, gap)))
        for name in ("status", "dropped", "retained"):
            assert np.array_equal(getattr(rd, name), getattr(rt, name)), f"step {step}: {name}"
        for s, c, st in zip(ids, counts, rt.status):
            big += st == LIVE_EBIG
            at[s] += c if st == 0 else 0                              # a refused run is not fed again
        for name in ("first_sample", "totals", "packets", "bytes"):
            assert np.array_equal(getattr(dev, name), getattr(twin, name)), f"step {step}: {name}"
        assert dev.stats == twin.stats
        for x, y, name in zip(dev.snapshot(), twin.snapshot(), "first status begin out_end totals data offsets".split()):
            assert np.array_equal(x, y), f"step {step}: snapshot {name}"
    assert big > 0 and dev.stats["trims_by_packets"] > 0 and dev.stats["trims_by_bytes"] > 0
    assert dev.packets[3] == 0 and dev.totals[3] == 0
    # a device store in the twin's calls, a host store in the device's
    z = np.zeros(1, np.int64)
    assert v.lib.vbm_host_live_store_append(dev._h, 0, None, None, None, z.ctypes.data, 0, None, None, None, None, None,
                                            None) == EINVAL
    assert v.lib.vbm_host_live_store_restart(dev._h, 0, None) == EINVAL
    got = np.zeros(1, np.int32)
    assert v.lib.vbm_synthesis_ranges(dec._h, twin._h, 0, None, None, None, None, 0, got.ctypes.data, None) == EINVAL
    for x in (dev, twin, dec, ds):
        x.close()


# ---- 2. windows of a store fed from an OggFeed -----------------------------------------------------------------------
@pytest.mark.parametrize("halfrate", [False, True])
@pytest.mark.parametrize("max_packets", [4096, 16])
def test_windows_equal_the_linear_decode(cuda, material, halfrate, max_packets):
    _, ds, _, files = material
    dec = v.Decoder(ds, 3, 1024, halfrate=halfrate)
    store = v.LiveRangeStore(dec, 3, max_packets, 1 << 20)
    feed = v.OggFeed(3, 3 * 8192)
    lin, rng = Linear(3), np.random.default_rng(17)
    at, turn, checked, early = [0, 0, 0], 0, 0, 0
    while any(a < len(f) for a, f in zip(at, files)):
        ids = [s for s in range(3) if at[s] < len(files[s])]
        sizes = [(777, 0, 4096)[(turn + s) % 3] for s in ids]
        turn += 1
        r = feed.push(ids, [files[s][at[s]:at[s] + n] for s, n in zip(ids, sizes)],
                      end=[at[s] + n >= len(files[s]) for s, n in zip(ids, sizes)])
        for s, n in zip(ids, sizes):
            at[s] += n
        assert not any(r.status)
        live = np.flatnonzero(r.counts)
        if len(live):
            pcm, n, _, status = dec.synthesis_runs(r.ids[live], r.counts[live], r.payload, r.offsets,
                                                   granulepos=r.granulepos, eos=r.eos)
            lin.add(r.ids[live].tolist(), pcm, n)
        append_result(store, r, max_packets)
        a, b = check_windows(dec, store, lin, rng, range(3))
        checked, early = checked + a, early + b
    trims = store.stats["trims_by_packets"]
    assert checked > 100 and (trims > 0 and early > 0 if max_packets == 16 else trims == 0)
    assert np.array_equal(store.totals, [lin.of(s, 2).shape[1] for s in range(3)]) and store.totals.min() > 20000 >> halfrate
    for x in (feed, store, dec):
        x.close()


# ---- 3. gap marks -----------------------------------------------------------------------------------------------------
def test_gaps_on_the_device(cuda, material):
    _, ds, _, files = material
    pages = ogg_pages.split_pages(files[0])
    n = len(pages)
    assert n >= 6                                                      # pages 0 and 1 carry the headers
    lost, hurt = 2 + (n - 2) // 3, 2 + 2 * (n - 2) // 3
    pages[hurt][len(pages[hurt]) - 3] ^= 0x55                          # one audio page damaged: its CRC no longer holds
    mount = b"".join(bytes(p) for k, p in enumerate(pages) if k != lost)  # one audio page removed
    dec = v.Decoder(ds, 1, 1024)
    store = v.LiveRangeStore(dec, 1, 40, 1 << 20)
    feed = v.OggFeed(1, 8192, resync=True)
    lin, rng, marks, checked = Linear(1), np.random.default_rng(19), 0, 0
    for a in range(0, len(mount), 1500):
        for r in feed.push_all([0], [mount[a:a + 1500]], end=a + 1500 >= len(mount)):
            assert not any(r.status)
            if not r.counts[0]:
                continue
            marks += int(r.gap.sum().item())
            pcm, n, _, _ = dec.synthesis_runs(r.ids, r.counts, r.payload, r.offsets, granulepos=r.granulepos, eos=r.eos,
                                              gap=r.gap)
            lin.add([0], pcm, n)
            append_result(store, r, 40, gap=r.gap)
            checked += check_windows(dec, store, lin, rng, [0])[0]
    assert marks >= 1 and checked > 20 and store.stats["trims_by_packets"] > 0
    for x in (feed, store, dec):
        x.close()


# ---- 4. two classes of a mixed decoder -------------------------------------------------------------------------------
def test_mixed_classes_and_a_restart_into_the_other(cuda, material):
    _, ds2, pks, _ = material
    mono = v.Setup(1, 44100, 0.5)
    ds1 = v.DecodeSetup(v.header_packets(mono))
    pk1 = encoded(v, mono, 1.0, 55, cuda)
    md = v.MixedDecoder(2, 256, max_classes=2, max_channels=2, max_blocksize=2048)
    c1, c2 = md.add_class(ds1), md.add_class(ds2)
    store = v.LiveRangeStore(md, 2, 24, 1 << 20)
    with pytest.raises(v.VbmError):                                   # a slot without a class takes nothing
        store.append([0], [0], torch.zeros(0, dtype=torch.uint8, device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda))
    store.restart([0, 1], [c2, c1])
    want = {0: linear(v, ds2, pks[0], cuda), 1: linear(v, ds1, pk1, cuda), 2: linear(v, ds2, pks[2], cuda)}
    src = {0: pks[0], 1: pk1}
    channels, pos, rng, checked = {0: 2, 1: 1}, {0: 0, 1: 0}, np.random.default_rng(23), 0

    class Whole:                                                      # lin of check_windows: the fed part of the whole decode
        def of(self, sid, ch):
            return want[key[sid]][:, :int(store.totals[sid])]
    key = {0: 0, 1: 1}
    restarted = False
    while pos[0] < len(src[0]) or pos[1] < len(src[1]):
        ids = [s for s in (0, 1) if pos[s] < len(src[s])]
        counts = [min(int(rng.integers(0, 20)), len(src[s]) - pos[s]) for s in ids]
        rows = [p for s, c in zip(ids, counts) for p in src[s][pos[s]:pos[s] + c]]
        data = np.frombuffer(b"".join(p[0] for p in rows) or b"\0", np.uint8).copy()
        offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in rows])]).astype(np.int64)
        out = store.append(ids, counts, to_dev(data, cuda), to_dev(offs, cuda),
                           granulepos=to_dev(np.array([p[1] for p in rows], np.int64), cuda),
                           eos=to_dev(np.array([p[2] for p in rows], np.uint8), cuda))
        assert not out.status.any()
        for s, c in zip(ids, counts):
            pos[s] += c
        checked += check_windows(md, store, Whole(), rng, [0, 1], channels)[0]
        if not restarted and pos[1] == len(src[1]):                  # slot 1 goes from the mono class into the stereo one
            store.restart([1], [c2])
            assert store.totals[1] == store.first_sample[1] == 0
            src[1], pos[1], key[1], channels[1], restarted = pks[2], 0, 2, 2, True
    assert restarted and checked > 100 and store.stats["trims_by_packets"] > 0
    assert store.totals[0] == want[0].shape[1] and store.totals[1] == want[2].shape[1]
    for x in (store, md, ds1):
        x.close()


# ---- 5. cuts ----------------------------------------------------------------------------------------------------------
def test_cuts_of_a_live_store(cuda, material):
    setup, ds, pks, _ = material
    from vorbis_aotuv_lancer_amd.stream import header_pages
    dec = v.Decoder(ds, 2, 1024)
    store = v.LiveRangeStore(dec, 2, 48, 1 << 20)
    rng = np.random.default_rng(29)
    for sid, pk in enumerate(pks[::2]):
        for a in range(0, len(pk), 13):
            rows = pk[a:a + 13]
            data = np.frombuffer(b"".join(p[0] for p in rows), np.uint8).copy()
            offs = np.concatenate([[0], np.cumsum([len(p[0]) for p in rows])]).astype(np.int64)
            out = store.append([sid], [len(rows)], to_dev(data, cuda), to_dev(offs, cuda),
                               granulepos=to_dev(np.array([p[1] for p in rows], np.int64), cuda),
                               eos=to_dev(np.array([p[2] for p in rows], np.uint8), cuda))
            assert out.status[0] == 0
    assert store.stats["trims_by_packets"] > 0 and store.first_sample.min() > 0
    hdr = header_pages(v.header_packets(setup), 0)
    ids, starts, lengths = [], [], []
    for sid in (0, 1):
        lo, T = int(store.first_sample[sid]), int(store.totals[sid])
        w = [(lo, 2000), (lo + 300, T - lo - 300), (T - 900, 5000), (lo - 1, 500)]       # the last: before first_sample
        w += [(lo + int(rng.integers(0, (T - lo) // 2)), int(rng.integers(500, (T - lo) // 2))) for _ in range(2)]
        for s0, L in w:
            ids.append(sid), starts.append(s0), lengths.append(L)
    n = len(ids)
    cutter = v.OggCutter(n, 1 << 20, len(hdr))
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
    off, stat, gs, gl = cutter.cut(store, ids, starts, lengths, [hdr] * n, out=buf)
    off, stat, raw = off.cpu().numpy(), stat.cpu().numpy(), buf.cpu().numpy().tobytes()
    assert not stat.any()
    clips = [raw[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
    early = [r for r in range(n) if starts[r] < store.first_sample[ids[r]]]
    assert len(early) == 2 and all(clips[r] == b"" and gl[r] == 0 for r in early)
    kept = [r for r in range(n) if r not in early]
    assert all(gl[r] > 0 and clips[r] for r in kept)
    pcm, got = ranges(dec, store, [ids[r] for r in kept], [int(gs[r]) for r in kept], [int(gl[r]) for r in kept])
    for k, (r, (clip_pcm, rate)) in enumerate(zip(kept, v.decode_ogg([clips[r] for r in kept]))):
        assert got[k] == gl[r] == clip_pcm.shape[1] and rate == 44100
        assert np.array_equal(clip_pcm.cpu().numpy(), pcm[k, :, :got[k]]), f"clip {r}"
    # the host cutter over a snapshot writes the same files
    host = v.OggCutter(len(kept), 1 << 20, len(hdr), host=True)
    hbuf = np.zeros(1 << 20, np.uint8)
    hoff, hstat, hgs, hgl = host.cut(store.snapshot(), [ids[r] for r in kept], [starts[r] for r in kept],
                                     [lengths[r] for r in kept], [hdr] * len(kept), serialnos=kept, out=hbuf)
    assert not hstat.any()
    assert [hbuf[int(a):int(b)].tobytes() for a, b in zip(hoff[:-1], hoff[1:])] == [clips[r] for r in kept]
    assert np.array_equal(hgs, gs[kept]) and np.array_equal(hgl, gl[kept])
    # a half-rate store is refused, as a half-rate RangeStore is
    hdec = v.Decoder(ds, 1, 64, halfrate=True)
    hstore = v.LiveRangeStore(hdec, 1, 8, 1024)
    with pytest.raises(v.VbmError):
        cutter.cut(hstore, [0], [0], [10], [hdr], out=buf)
    for x in (hstore, hdec, host, cutter, store, dec):
        x.close()
