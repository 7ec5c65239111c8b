"""Corpus and helpers of tests/test_decode_mixed_gpu.py: header classes (synthetic ones from tests/vorbis_model.py, real
ones from encode_ogg), streams of them, and a player that runs one script of binds and decode calls twice: on one
MixedDecoder, and on the yardstick, a single-class Decoder per class fed the same packets of the same streams in the
same calls.  Every comparison is exact."""
import functools

import numpy as np
import torch

from tests import vorbis_model as vm
from tests.test_decoder_model_cpu import fromdB

FILL = -77.25            # what the output buffers hold before a call: not a sample value of any corpus stream
SEQ = vm.SEQUENCES[0]    # short->short, short->long, long->short and long->long


class Class:
    """one header class: .headers, .ch, .bs, .model (synthetic classes only); .ds is opened by the tests"""

    def __init__(self, headers, ch, bs, model=None):
        self.headers, self.ch, self.bs, self.model = headers, ch, bs, model

    def W(self, packet):
        """the block-size flag of a writer-made packet of a synthetic class: that of the mode its first bits name"""
        head = int.from_bytes(packet[:2], "little")
        assert head & 1 == 0
        return self.model.s["modes"][(head >> 1) & ((1 << self.model.modebits) - 1)][0]


@functools.lru_cache(maxsize=None)
def synthetic(ch, bs, seed=0):
    """a synthetic class of `ch` channels and block sizes `bs` whose writer-made packets are loud (as vm.pcm_setup)"""
    setup, coding = vm.gen_setup(6000 + 97 * ch + bs[0] // 64 + bs[1] + seed, ch=ch, bs=bs, res_types=(1, 2),
                                 min_exp=0, coupling="pairs" if ch > 1 else "none",
                                 res_kw=dict(bad_classwords=False, masks=[1, 3, 5, 7]))
    return Class(vm.pack_headers(setup, coding), ch, bs, vm.Model(setup, fromdB()))


@functools.lru_cache(maxsize=None)
def stream(ch, bs, seq=SEQ, seed=0, contrary=False):
    """one stream [(packet, granulepos, eos)] of synthetic(ch, bs) with the block-size sequence `seq`; the last packet
    carries a granule position 37 samples short of the length, and the end-of-stream flag.  contrary: the packets' own
    lW / nW bits contradict their neighbours (vm.pcm_streams' second stream)"""
    seqs = [seq, seq] if contrary else [seq]
    return tuple(vm.pcm_streams(synthetic(ch, bs).model, 9000 + seed, sequences=seqs)[-1])


def sequence(n):
    """a block-size sequence of n packets with every transition"""
    return (SEQ * (n // len(SEQ) + 1))[:n]


def ogg_packets(blob):
    """an .ogg file -> (headers, [(packet, granulepos, eos)])"""
    import vorbis_aotuv_lancer_amd as v
    headers, data, offsets, gp, eos = v.demux_ogg(blob)
    data = np.asarray(data, np.uint8).tobytes()
    return headers, [(data[int(a):int(b)], int(g), int(e)) for a, b, g, e in zip(offsets[:-1], offsets[1:], gp, eos)]


# ---- scripts --------------------------------------------------------------------------------------------------------
# A script is a list of events:
#   ("add", c)                        class c of the test's class list joins the mixed decoder's table
#   ("bind", [stream ids], [c ...])   the streams are of these classes from here on, and restart
#   ("batch", [(stream id, (packet, granulepos, eos)) ...])                 one synthesis_batch call
#   ("runs", [(stream id, [(packet, granulepos, eos[, gap]) ...]) ...])     one synthesis_runs call
def _batch_inputs(rows, dev):
    from tests.test_decoder_gpu import rows_tensor
    pk, nb = rows_tensor([p[0] for _, p in rows], dev)
    gp = torch.tensor([p[1] for _, p in rows], dtype=torch.int64, device=dev)
    eo = torch.tensor([p[2] for _, p in rows], dtype=torch.uint8, device=dev)
    return pk, nb, gp, eo


def _runs_inputs(runs, dev):
    flat = [p for _, r in runs for p in r]
    data = np.frombuffer(b"".join(p[0] for p in flat), np.uint8).copy()
    offs = np.zeros(len(flat) + 1, np.int64)
    offs[1:] = np.cumsum([len(p[0]) for p in flat])
    gap = np.array([p[3] if len(p) > 3 else 0 for p in flat], np.uint8)
    up = lambda a: torch.from_numpy(a).to(dev)                       # noqa: E731
    return (up(data) if len(data) else torch.zeros(0, dtype=torch.uint8, device=dev), up(offs),
            up(np.array([p[1] for p in flat], np.int64)), up(np.array([p[2] for p in flat], np.uint8)),
            up(gap) if gap.any() else None)


class Player:
    """Runs a script.  Every input tensor is made before the first call and every output is read after the last one,
    so the calls follow each other with no host wait in between.  .result[stream id] is the list, one entry per call
    the stream took part in, of (pcm [channels, n] numpy, samples [packets], status [packets])."""

    def __init__(self, v, classes, S, cap, dev, halfrate=False):
        self.v, self.classes, self.S, self.cap, self.dev, self.halfrate = v, classes, S, cap, dev, halfrate
        self.of = {}                                                 # stream id -> class index
        self.blocks = []                                             # per decode call: {transform size: blocks}

    def play(self, script):
        prepared = []
        for ev in script:
            if ev[0] == "batch":
                prepared.append(_batch_inputs(ev[1], self.dev))
            elif ev[0] == "runs":
                prepared.append(_runs_inputs(ev[1], self.dev))
            else:
                prepared.append(None)
        torch.cuda.synchronize()
        pending = []
        for ev, inp in zip(script, prepared):
            if ev[0] == "add":
                self.add(ev[1])
            elif ev[0] == "bind":
                self.bind(ev[1], ev[2])
                self.of.update(zip(ev[1], ev[2]))
            else:
                pending += self.call(ev[0], ev[1], inp)
        self.result = {}
        for sid, ch, pcm, n, samples, status in pending:            # the one wait is the first .cpu() here
            n = int(n)
            full = pcm.cpu().numpy()
            assert np.all(full[ch:] == FILL) and np.all(full[:ch, n:] == FILL), f"stream {sid}: written outside its PCM"
            self.result.setdefault(sid, []).append((full[:ch, :n], samples.cpu().tolist(), status.cpu().tolist()))
        self.close()
        return self.result

    def out(self, n, channels, stride, P=None):
        dev = self.dev
        pcm = torch.full((n, channels, stride), FILL, dtype=torch.float32, device=dev)
        ints = [torch.empty(k, dtype=torch.int32, device=dev) for k in ([n, n] if P is None else [n, P, P])]
        return (pcm, *ints)

    def call_on(self, dec, kind, ids, rows, inp, chans, stride):
        """one call of `dec` over rows [(stream id, packet or run)] under the stream ids `ids` -> pending entries"""
        if kind == "batch":
            pk, nb, gp, eo = inp
            pcm, samples, status = dec.synthesis_batch(ids, pk, nb, granulepos=gp, eos=eo,
                                                       out=self.out(len(ids), dec.channels, dec.row))
            return [(sid, chans[r], pcm[r], samples[r], samples[r:r + 1], status[r:r + 1])
                    for r, (sid, _) in enumerate(rows)]
        data, offs, gp, eo, gap = inp
        counts = [len(r) for _, r in rows]
        pcm, rs, samples, status = dec.synthesis_runs(ids, counts, data, offs, granulepos=gp, eos=eo, gap=gap,
                                                      out=self.out(len(ids), dec.channels, stride, sum(counts)))
        at = np.cumsum([0] + counts)
        return [(sid, chans[r], pcm[r], rs[r], samples[at[r]:at[r + 1]], status[at[r]:at[r + 1]])
                for r, (sid, _) in enumerate(rows)]

    def row(self, c):
        return self.classes[c].bs[1] // (4 if self.halfrate else 2)

    def count_blocks(self, kind, rows):
        """.blocks gets, for a call whose packets are all writer-made ones of synthetic classes: per block size the
        (class, W, channels) of every row of it"""
        sizes = {}
        for sid, r in rows:
            k = self.classes[self.of[sid]]
            if k.model is None:
                return
            for p in ([r] if kind == "batch" else r):
                W = k.W(p[0])
                sizes.setdefault(k.bs[W], []).append((self.of[sid], W, k.ch))
        self.blocks.append(sizes)


class Mixed(Player):
    """the script on one MixedDecoder"""

    def __init__(self, v, classes, S, cap, dev, halfrate=False, count=False, **caps):
        super().__init__(v, classes, S, cap, dev, halfrate)
        self.md = v.MixedDecoder(S, cap, halfrate=halfrate, **caps)
        self.cid, self.count = {}, count

    def add(self, c):
        self.cid[c] = self.md.add_class(self.classes[c].ds)

    def bind(self, ids, cs):
        self.md.bind(ids, [self.cid[c] for c in cs])

    def call(self, kind, rows, inp):
        ids = [sid for sid, _ in rows]
        if self.count:
            self.count_blocks(kind, rows)
        chans = [self.classes[self.of[s]].ch for s in ids]
        assert chans == self.md.channels_of(ids)
        stride = max([1] + [len(r) * self.row(self.of[s]) for s, r in rows]) if kind == "runs" else None
        return self.call_on(self.md, kind, ids, rows, inp, chans, stride)

    def close(self):
        self.md.close()


class PerClass(Player):
    """the yardstick: one single-class Decoder per class, each taking its own streams' rows of every call"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.dec = {}

    def add(self, c):
        self.dec[c] = self.v.Decoder(self.classes[c].ds, self.S, self.cap, halfrate=self.halfrate)

    def bind(self, ids, cs):
        for c in sorted(set(cs)):
            self.dec[c].restart_streams([s for s, k in zip(ids, cs) if k == c])

    def call(self, kind, rows, inp):
        out = []
        for c in sorted({self.of[s] for s, _ in rows}):
            mine = [(s, r) for s, r in rows if self.of[s] == c]
            sub = _batch_inputs(mine, self.dev) if kind == "batch" else _runs_inputs(mine, self.dev)
            stride = max([1] + [len(r) * self.row(c) for _, r in mine]) if kind == "runs" else None
            out += self.call_on(self.dec[c], kind, [s for s, _ in mine], mine, sub, [self.classes[c].ch] * len(mine),
                                stride)
        return out

    def close(self):
        for d in self.dec.values():
            d.close()


def same(got, want):
    """the results of two players: the same streams, and per stream and call equal PCM, samples and status"""
    assert sorted(got) == sorted(want)
    total = 0
    for sid in want:
        assert len(got[sid]) == len(want[sid])
        for k, ((p, sm, st), (wp, wsm, wst)) in enumerate(zip(got[sid], want[sid])):
            assert sm == wsm and st == wst, f"stream {sid}, call {k}: samples or status"
            assert p.shape == wp.shape and np.array_equal(p, wp), f"stream {sid}, call {k}: PCM"
            total += p.shape[1]
    return total


def both(v, classes, script, S, cap, dev, halfrate=False, count=False, **caps):
    """the script on a MixedDecoder and on the yardstick, compared -> the Mixed player (its .result, .blocks)"""
    for k in classes:
        k.ds = v.DecodeSetup(k.headers)
    try:
        m = Mixed(v, classes, S, cap, dev, halfrate, count, **caps)
        got = m.play(script)
        want = PerClass(v, classes, S, cap, dev, halfrate).play(script)
        m.samples = same(got, want)
        assert m.samples > 0
    finally:
        for k in classes:
            k.ds.close()
    return m
