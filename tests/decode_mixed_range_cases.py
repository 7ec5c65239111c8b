"""Streams, windows and players of tests/test_decode_mixed_ranges_gpu.py and tests/test_decode_mixed_index_cpu.py: range
stores and the index over several header classes.  The streams are writer-made ones of tests/decode_mixed_cases.py's
synthetic classes; the yardstick of every range call is the single-class path, one Decoder + RangeStore +
synthesis_ranges per class over the same windows of the same streams.  Every comparison is exact."""
import numpy as np

from tests import decode_mixed_cases as M
from tests.decode_packets import as_stream, join

# classes that collide on transform sizes: 512 is the long block of one, both blocks of another and the short block of
# a third; 4096 is both blocks of the widest class
COLLIDING = [(1, (256, 512)), (2, (512, 512)), (3, (512, 4096)), (7, (4096, 4096)), (2, (1024, 2048))]
NPACKETS = 12


def csr(streams):
    """[(class, packets)] -> (data, offsets, granulepos, eos, stream_packets) of all of them back to back"""
    return join([as_stream(pk) for _, pk in streams])


def range_streams():
    """-> (classes, [(class index, packets)]): eight streams of the five COLLIDING classes, 12 packets each with every
    block transition, the last packet with a trimming granule position and e_o_s; neighbours are of different classes"""
    classes = [M.synthetic(ch, bs) for ch, bs in COLLIDING]
    of = [0, 1, 2, 3, 4, 1, 3, 0]
    return classes, [(c, list(M.stream(*COLLIDING[c], seq=M.sequence(NPACKETS), seed=s))) for s, c in enumerate(of)]


def index_streams():
    """-> (classes, [(class index, packets)]) of the index tests: streams 0-3 of four classes (one block of the scan
    kernel), seven streams of the five COLLIDING classes in all, then one of 130 packets of (256, 256) (two chunk
    carries), one with a granule position below -1 on a valid packet (the single-lane walk), an empty one, and one
    with a truncated and a header packet inside"""
    classes = [M.synthetic(ch, bs) for ch, bs in COLLIDING] + [M.synthetic(1, (256, 256))]
    of = [0, 1, 2, 3, 4, 2, 0]
    streams = [(c, list(M.stream(*COLLIDING[c], seq=M.sequence(NPACKETS), seed=20 + s))) for s, c in enumerate(of)]
    streams.append((5, list(M.stream(1, (256, 256), seq=M.sequence(130), seed=31))))
    low = list(M.stream(*COLLIDING[4], seq=M.sequence(NPACKETS), seed=32))
    low[3] = (low[3][0], -5, 0)
    streams.append((4, low))
    streams.append((1, []))
    broken = list(M.stream(*COLLIDING[1], seq=M.sequence(NPACKETS), seed=33))
    broken[4] = (b"", -1, 0)
    broken[7] = (b"\x03vorbis", -1, 0)
    streams.append((1, broken))
    return classes, streams


def host_index(v, classes_ds, streams, halfrate):
    """per stream decode_index_scan_host with its class's setup -> [(status, begin, end, out_start, total)]"""
    out = []
    for c, pk in streams:
        data, offs, gp, eo = as_stream(pk)
        st, b, e, o, t = v.decode_index_scan_host(classes_ds[c], data, offs, gp, eo, halfrate=halfrate)
        out.append((st, b, e, o, int(t[0])))
    return out


def windows_of(index):
    """the windows of every stream of `index` (host_index's), kind by kind over all streams, so that neighbours in the
    call are of different streams: the whole stream, one that starts and ends mid-packet, one inside a single packet,
    one straddling the end (got < length), one past the end (got == 0), one of length 0, two that overlap
    -> [(stream, start, length)]"""
    kinds = []
    for s, (st, b, e, o, T) in enumerate(index):
        n = e - b
        inner = int(np.argmax(n >= 20))
        assert n[inner] >= 20 and T > 400
        kinds.append([(s, 0, T), (s, int(o[3]) + 5, int(o[8]) + 7 - int(o[3]) - 5), (s, int(o[inner]) + 3, 10),
                      (s, T - 50, 200), (s, T + 10, 64), (s, 5, 0), (s, 100, 250), (s, 250, 150)])
    return [w for k in range(len(kinds[0])) for w in (kind[k] for kind in kinds)]


def plan_calls(first, status, out_end, totals, cap, windows):
    """vbm_plan_ranges' packing (csrc/range_plan.h) -> per sub-call the list of its pieces' streams: a piece is a
    pre-roll row and up to cap - 1 rows, and a sub-call closes when the next piece would pass cap rows or cap ranges"""
    calls, rows, r0 = [[]], 0, None
    for r, (i, s, length) in enumerate(windows):
        got = max(0, min(totals[i] - s, length))
        if got == 0:
            continue
        a, b = int(first[i]), int(first[i + 1])
        k = a + int(np.searchsorted(out_end[a:b], s, side="right"))
        m = a + int(np.searchsorted(out_end[a:b], s + got - 1, side="right"))
        pre = k - 1
        while status[pre] != 0:
            pre -= 1
        f = pre + 1
        while f <= m:
            count = min(m - f + 1, cap - 1)
            if rows + count + 1 > cap or (r0 is not None and r - r0 >= cap):
                calls.append([])
                rows, r0 = 0, None
            if r0 is None:
                r0 = r
            calls[-1].append(i)
            rows += count + 1
            f += count
    return [c for c in calls if c]


def mixed_ranges(v, md, store, windows, dev, stride):
    """one synthesis_ranges call of the mixed decoder into a FILL_PLAYER buffer -> (pcm tensor, got); nothing is awaited"""
    import torch
    pcm = torch.full((len(windows), md.channels, stride), M.FILL_PLAYER, dtype=torch.float32, device=dev)
    _, got = md.synthesis_ranges(store, [w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows],
                                 out=pcm)
    return pcm, got


class Yardstick:
    """one Decoder and one RangeStore per class over the streams of that class"""

    def __init__(self, v, classes_ds, streams, cap, halfrate=False):
        self.v, self.of = v, [c for c, _ in streams]
        self.local, self.dec, self.store = {}, {}, {}
        for c in sorted(set(self.of)):
            mine = [s for s, k in enumerate(self.of) if k == c]
            self.local.update({s: j for j, s in enumerate(mine)})
            self.dec[c] = v.Decoder(classes_ds[c], 1, cap, halfrate=halfrate)
            self.store[c] = v.RangeStore(self.dec[c], [as_stream(streams[s][1]) for s in mine])

    def ranges(self, windows, dev, stride):
        """-> per window (pcm [channels, stride] numpy, got), each class's windows in one call of its own"""
        import torch
        out, pending = [None] * len(windows), []
        for c, dec in self.dec.items():
            rows = [r for r, w in enumerate(windows) if self.of[w[0]] == c]
            if not rows:
                continue
            pcm = torch.full((len(rows), dec.channels, stride), M.FILL_PLAYER, dtype=torch.float32, device=dev)
            _, got = dec.synthesis_ranges(self.store[c], [self.local[windows[r][0]] for r in rows],
                                          [windows[r][1] for r in rows], [windows[r][2] for r in rows], out=pcm)
            pending.append((rows, pcm, got))
        for rows, pcm, got in pending:
            pcm = pcm.cpu().numpy()
            for j, r in enumerate(rows):
                out[r] = (pcm[j], int(got[j]))
        return out

    def close(self):
        for x in list(self.store.values()) + list(self.dec.values()):
            x.close()


def same_ranges(pcm, got, want, channels):
    """the mixed call's (pcm [n, max channels, stride] numpy, got) against Yardstick.ranges' rows: got equal, the
    class's channels equal over the full stride (so the fill is intact past got), the other channels all fill"""
    written = 0
    for r, (wp, wg) in enumerate(want):
        ch = channels[r]
        assert int(got[r]) == wg, f"window {r}: got"
        assert wp.shape == (ch, pcm.shape[2])
        assert np.array_equal(pcm[r, :ch], wp), f"window {r}: PCM"
        assert np.all(pcm[r, ch:] == M.FILL_PLAYER), f"window {r}: written past its channels"
        assert np.all(wp[:, wg:] == M.FILL_PLAYER)
        written += wg
    return written
