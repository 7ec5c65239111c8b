"""Packet schedules for the Ogg mux tests (test_ogg_mux_cpu.py, test_ogg_mux_gpu.py) and the yardstick they are checked
against: the host writer (OggStream), driven per stream as write_ogg drives it — packetin, then pages() after every
packet, pages(flush=True) where the call flushes."""
import numpy as np

import vorbis_aotuv_lancer_amd as v
from tests.ogg_pages import random_bytes as payload

INFO = np.dtype({"names": ["stream", "block_mode", "lW", "W", "nW", "eos", "granulepos", "packetno"],
                 "formats": ["<i4"] * 6 + ["<i8", "<i8"]})
assert INFO.itemsize == 40


# ---- per-stream schedules: a list of steps, each a list of (size, eos) packets, or "restart" ------------------------

def sched_sizes(M):
    return [[(n, False)] for n in (0, 1, 254, 255, 256, 510, min(M, 4097 + 300))] + [[(7, True)]]


def sched_ones(R):
    """300 one-byte packets: a page is forced at 255 segments"""
    out, left = [], 300
    while left:
        k = min(R, left)
        out.append([(1, False)] * k)
        left -= k
    return out + [[(3, True)]]


def sched_253_600(R):
    """253 one-byte packets, a 600-byte packet, then three more with e_o_s on the last"""
    out, left = [], 253
    while left:
        k = min(R, left)
        out.append([(1, False)] * k)
        left -= k
    return out + [[(600, False)], [(40, False), (40, False)], [(40, True)]]


def sched_big(M):
    return [[(30, False)], [(M, False)], [(31, False)], [(M, False), (5, False)], [(9, True)]]


def sched_restart(rng, M):
    a = [[(int(rng.integers(0, 900)), False)] for _ in range(6)] + [[(100, True)]]
    b = [[(int(rng.integers(0, min(M, 5000))), False)] for _ in range(5)] + [[(64, False), (65, True)]]
    return a + ["restart"] + b


def sched_random(rng, M, R, steps=18):
    kind = int(rng.integers(0, 4))
    out = []
    for t in range(steps):
        k = int(rng.integers(0, [3, 2, R + 1, 2][kind]))
        hi = [700, min(M, 6000), 4, 300][kind]
        out.append([(int(rng.integers(0, hi + 1)), False) for _ in range(k)])
    out.append([(int(rng.integers(0, 500)), True)])
    return out


def directed(rng, M, R):
    return [sched_sizes(M), sched_ones(R), sched_253_600(R), sched_big(M), sched_restart(rng, M), [[]] * 4 + sched_sizes(M),
            sched_random(rng, M, R)]


class Case:
    """`nstreams` schedules zipped into calls: call t carries step t - delay[s] of every stream s, rows shuffled across
    streams and interleaved with empty rows.  flush_at: calls that flush."""

    def __init__(self, scheds, M, seed, flush_at=(), delays=None):
        self.scheds, self.M, self.seed, self.flush_at = scheds, M, seed, set(flush_at)
        self.n = len(scheds)
        self.delays = delays if delays is not None else [s % 3 for s in range(self.n)]
        self.ncalls = max(len(sc) + d for sc, d in zip(scheds, self.delays))

    def steps(self):
        """-> per call: (restarts [(stream, serialno)], rows [(stream, bytes, granulepos, eos, packetno)], flush)"""
        rng = np.random.default_rng(self.seed)
        pno = [3] * self.n
        gp = [0] * self.n
        gen = [0] * self.n
        for t in range(self.ncalls):
            restarts, rows = [], []
            for s in range(self.n):
                k = t - self.delays[s]
                if k < 0 or k >= len(self.scheds[s]):
                    continue
                step = self.scheds[s][k]
                if isinstance(step, str):
                    gen[s] += 1
                    pno[s], gp[s] = 3, 0
                    restarts.append((s, 1000 * gen[s] + s))
                    continue
                for size, eos in step:
                    gp[s] += 64 + size
                    rows.append((s, payload(rng, size), gp[s], eos, pno[s]))
                    pno[s] += 1
            order = rng.permutation(len(rows))
            yield restarts, [rows[i] for i in order], t in self.flush_at, np.random.default_rng([self.seed, t])


def pack_rows(rows, stride, rng=None, holes=True):
    """rows -> (info records, packets uint8 [n, stride], nbytes int32 [n]); with holes, empty rows are mixed in the way a
    device-built call leaves them (length -2, stream -1)"""
    slots = list(range(len(rows)))
    n = len(rows)
    if holes and rng is not None and n:
        n = len(rows) + int(rng.integers(0, 4))
        slots = sorted(rng.choice(n, len(rows), replace=False).tolist())
    info = np.zeros(n, INFO)
    info["stream"] = -1
    nbytes = np.full(n, -2, np.int32)
    packets = np.zeros((n, stride), np.uint8)
    for slot, (s, data, gp, eos, pno) in zip(slots, rows):
        info[slot] = (s, 3, 1, 1, 1, int(eos), gp, pno)
        nbytes[slot] = len(data)
        packets[slot, :len(data)] = np.frombuffer(data, np.uint8)
    return info, packets, nbytes


class Writer:
    """the yardstick: one host OggStream per slot"""

    def __init__(self, setup, nstreams, comments=()):
        self.setup, self.comments = setup, comments
        self.os = [None] * nstreams
        self.dead = [True] * nstreams
        self.headers = v.header_packets(setup, comments)

    def start(self, s, serialno):
        if self.os[s] is not None:
            self.os[s].close()
        os_ = self.os[s] = v.OggStream(int(np.int32(np.uint32(serialno))))
        self.dead[s] = False
        for h in self.headers:
            os_.packetin(h, 0)
        return b"".join(os_.pages(flush=True))

    def call(self, rows, flush):
        """-> (bytes per stream of this call, status per stream)"""
        n = len(self.os)
        out, status = [b""] * n, [0] * n
        by = {}
        for s, data, gp, eos, pno in rows:
            by.setdefault(s, []).append((pno, data, gp, eos))
        for s in range(n):
            got = []
            for pno, data, gp, eos in sorted(by.get(s, []), key=lambda r: r[0]):
                if status[s]:
                    break
                if self.os[s] is None or self.dead[s]:
                    status[s] = v.OggMux.ESTATE
                    break
                self.os[s].packetin(data, gp, eos)
                self.dead[s] = bool(eos)
                got += self.os[s].pages()
            if flush and self.os[s] is not None:
                got += self.os[s].pages(flush=True)
            out[s] = b"".join(got)
        return out, status

    def close(self):
        for o in self.os:
            if o is not None:
                o.close()


def run_case(case, mux_call, start_call, setup, stride=None):
    """Drive `case` through mux_call(info, packets, nbytes, flush) -> (out, offsets, status) as numpy, and through the
    host writer; assert equal bytes, offsets and status call by call.  Returns the bytes of every stream (headers
    included, restarts concatenated)."""
    w = Writer(setup, case.n)
    total = [b""] * case.n
    hdr = start_call(list(range(case.n)), list(range(case.n)))
    for s in range(case.n):
        assert hdr[s] == w.start(s, s), f"header pages of stream {s}"
        total[s] += hdr[s]
    for t, (restarts, rows, flush, rng) in enumerate(case.steps()):
        if restarts:
            hdr = start_call([s for s, _ in restarts], [sn for _, sn in restarts])
            for (s, sn), h in zip(restarts, hdr):
                assert h == w.start(s, sn), f"header pages of restarted stream {s}"
                total[s] += h
        info, packets, nbytes = pack_rows(rows, stride or case.M, rng)
        out, offsets, status = mux_call(info, packets, nbytes, flush)
        want, wstatus = w.call(rows, flush)
        assert offsets[0] == 0 and len(offsets) == case.n + 1
        assert list(status[:case.n]) == wstatus, f"call {t}: status"
        assert status[case.n] == 0
        for s in range(case.n):
            got = bytes(out[offsets[s]:offsets[s + 1]])
            assert got == want[s], f"call {t}, stream {s}: {len(got)} bytes, the host writer made {len(want[s])}"
            total[s] += got
    w.close()
    return total
