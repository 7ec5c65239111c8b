"""Corpus and helpers of tests/test_decode_mixed_gpu.py: header classes (synthetic ones from tests/vorbis_model.py, real
ones from encode_ogg), streams of them, and a player that runs one script of binds and decode calls twice: on one
MixedDecoder, and on the yardstick, a single-class Decoder per class fed the same packets of the same streams in the
same calls.  Every comparison is exact."""
import functools

import numpy as np
import torch

from tests import vorbis_model as vm
from tests.decode_calls import FILL_PLAYER, batch_inputs, runs_inputs
from tests.decode_packets import family as model_family
from tests.decode_packets import fromdB

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


# ---- the generated corpus (vm.CORPUS) as classes ----------------------------------------------------------------------
SILENT = "pair_2048_2048_end_le_begin"      # the family whose residue range is empty: every spectrum is zero


@functools.lru_cache(maxsize=None)
def family(k):
    """vm.CORPUS[k] as a Class, with .name, .setup (the dict), .packets (the bytes of vm.corpus_packets) and per packet
    the model's .status and .info, and .loud: its model spectrum is nonzero"""
    setup, _, headers, _, rows, _, _ = model_family(k)
    c = Class(headers, setup["channels"], tuple(setup["blocksizes"]), vm.Model(setup, fromdB()))
    c.name, c.setup = vm.CORPUS[k][0], setup
    c.packets = [p for _, p, _ in rows]
    c.status = [r["status"] for _, _, r in rows]
    c.info = [r["info"] for _, _, r in rows]
    c.loud = [bool(r["spectrum"].any()) for _, _, r in rows]
    return c


def family_named(name):
    return family([n for n, _ in vm.CORPUS].index(name))


@functools.lru_cache(maxsize=None)
def whole(k, seed=0):
    """(a, b): whole writer-made loud packets of family k, one of each block flag the family has, the short one first;
    the same packet twice where the family has one flag"""
    c = family(k)
    pw = vm.PacketWriter(c.model, np.random.default_rng(7100 + 131 * seed + k))
    modes = c.setup["modes"]
    made = []
    for f in sorted({md[0] for md in modes}):
        mine = [i for i, md in enumerate(modes) if md[0] == f]
        made.append(pw.packet(mine[seed % len(mine)], loud=True))
    return made[0], made[-1]


def family_stream(k, seed, seq=SEQ):
    """a stream of family k that follows the block-size sequence with whole(k, seed)'s two packets"""
    a, b = whole(k, seed)
    return [(b if c == "L" else a, -1, 0) for c in seq]


def corpus_pick(loud=None, failing=None):
    """{family: [packet indices]}: all of them, or per family the first `loud` packets with a nonzero model spectrum
    (in the silent family: that decode) and the first `failing` ones that fail"""
    pick = {}
    for k in range(len(vm.CORPUS)):
        f = family(k)
        if loud is None:
            pick[k] = list(range(len(f.packets)))
            continue
        good = [i for i in range(len(f.packets)) if (f.status[i] == 0 if f.name == SILENT else f.loud[i])]
        bad = [i for i in range(len(f.packets)) if f.status[i] != 0][:failing]
        at = 1 + 5 * k % (loud - 1)         # the first failing one at a place of the family's own: good neighbours
        pick[k] = good[:at] + bad[:1] + good[at:loud] + bad[1:]
    return pick


def corpus_script(pick):
    """Every picked corpus packet p of every family as a stream of its own that plays [p, a, p, b], with (a, b) =
    whole(family): a synthesis_batch of all p, one of all a, and one synthesis_runs of every [p, b].  The rows of the
    first two calls go round-robin over the families, those of the third in the reverse of that order.
    -> (classes, script, {(family, packet index): stream id}, the round-robin order [(family, packet index)])"""
    fams = [family(k) for k in range(len(vm.CORPUS))]
    sid = {}
    for k in range(len(fams)):
        for i in pick[k]:
            sid[k, i] = len(sid)
    order = [(k, pick[k][j]) for j in range(max(len(p) for p in pick.values())) for k in range(len(fams))
             if j < len(pick[k])]
    row = lambda p: (p, -1, 0)                                       # noqa: E731
    script = [("add", k) for k in range(len(fams))]
    script.append(("bind", [sid[x] for x in order], [k for k, _ in order]))
    script.append(("batch", [(sid[k, i], row(fams[k].packets[i])) for k, i in order]))
    script.append(("batch", [(sid[k, i], row(whole(k)[0])) for k, i in order]))
    script.append(("runs", [(sid[k, i], [row(fams[k].packets[i]), row(whole(k)[1])]) for k, i in order[::-1]]))
    return fams, script, sid, order


def corpus_blocks(order):
    """{transform size: {family: blocks}} of the first call over `order`, from the model's info as count_blocks does:
    a row that decodes puts its channels on the list of its block size"""
    sizes = {}
    for k, i in order:
        f = family(k)
        if f.status[i] == 0:
            of = sizes.setdefault(f.bs[f.info[i][1]], {})
            of[k] = of.get(k, 0) + f.ch
    return sizes


def corpus_sandwiched(order):
    """the rows of the first call that fail between two rows of other families that decode"""
    ok = [family(k).status[i] == 0 for k, i in order]
    return [r for r in range(1, len(order) - 1)
            if not ok[r] and ok[r - 1] and ok[r + 1] and order[r - 1][0] != order[r][0] != order[r + 1][0]]


def class_bytes(setup):
    """the partition-class scratch one packet of this setup dict needs, before rounding (parse_setup's arithmetic: per
    residue the partitions of the largest block, for every channel in types 0 and 1)"""
    n, ch = setup["blocksizes"][1] // 2, setup["channels"]
    need = 1
    for r in setup["residues"]:
        size = n * ch if r["type"] == 2 else n
        length = min(r["end"], size) - r["begin"]
        if length > 0:
            need = max(need, length // r["grouping"] * (1 if r["type"] == 2 else ch))
    return need


# decoders whose caps a class meets exactly: (caps, corpus families, a synthetic class beside them or None)
CAPS = [
    (dict(max_channels=3, max_blocksize=256), ["pair_256_256_grouping1"], (1, (256, 256))),       # the class scratch
    (dict(max_channels=8, max_blocksize=512), ["modes_5_submaps_16", "group_dim4_ragged", "pair_256_512_res0"],
     (1, (256, 512))),                                                                            # channels, few bins
    (dict(max_channels=2, max_blocksize=4096), ["pair_4096_4096_single_books", "pair_512_4096_long_codewords",
                                                "pair_256_2048_maptype2", "modes_1"], None),      # bins, few channels
]
CAPS_ROWS = 9                               # more than one IMDCT group of 256-blocks at 3 channels, and no multiple


def caps_script(n):
    """CAPS[n] -> (classes, script, the class of every row): CAPS_ROWS streams of SEQ, the rows going round the classes
    from the last one on, so in CAPS[0] every row of the corpus family lies between two rows of the synthetic class;
    five steps of one packet per stream, then the rest in one runs call"""
    _, names, synth = CAPS[n]
    classes = [family_named(x) for x in names] + ([synthetic(*synth)] if synth else [])
    of = [(r + len(classes) - 1) % len(classes) for r in range(CAPS_ROWS)]
    index = [x for x, _ in vm.CORPUS]
    streams = {}
    for r, c in enumerate(of):
        if c < len(names):
            streams[r] = family_stream(index.index(names[c]), 1 + r // len(classes))
        else:
            streams[r] = list(stream(*synth, seed=r))
    script = [("add", c) for c in range(len(classes))] + [("bind", list(range(CAPS_ROWS)), of)]
    script += [("batch", [(s, pk[t]) for s, pk in streams.items()]) for t in range(5)]
    script.append(("runs", [(s, pk[5:]) for s, pk in streams.items()]))
    return classes, script, of


# ---- scripts --------------------------------------------------------------------------------------------------------
# A script is a list of events:
#   ("add", c)                        class c of the test's class list joins the mixed decoder's table
#   ("bind", [stream ids], [c ...])   the streams are of these classes from here on, and restart
#   ("batch", [(stream id, (packet, granulepos, eos)) ...])                 one synthesis_batch call
#   ("runs", [(stream id, [(packet, granulepos, eos[, gap]) ...]) ...])     one synthesis_runs call
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
                prepared.append(batch_inputs([p for _, p in ev[1]], self.dev))
            elif ev[0] == "runs":
                prepared.append(runs_inputs([r for _, r in ev[1]], self.dev))
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
        for meta, at, pcm, n, samples, status in pending:           # the one wait is the first .cpu() here
            pcm, n = pcm.cpu().numpy(), n.cpu().tolist()
            samples, status = samples.cpu().tolist(), status.cpu().tolist()
            for r, (sid, ch) in enumerate(meta):
                full = pcm[r]
                assert np.all(full[ch:] == FILL_PLAYER) and np.all(full[:ch, n[r]:] == FILL_PLAYER), \
                    f"stream {sid}: written outside its PCM"
                self.result.setdefault(sid, []).append((full[:ch, :n[r]], samples[at[r]:at[r + 1]],
                                                        status[at[r]:at[r + 1]]))
        self.close()
        return self.result

    def out(self, n, channels, stride, P=None):
        dev = self.dev
        pcm = torch.full((n, channels, stride), FILL_PLAYER, dtype=torch.float32, device=dev)
        ints = [torch.empty(k, dtype=torch.int32, device=dev) for k in ([n, n] if P is None else [n, P, P])]
        return (pcm, *ints)

    def call_on(self, dec, kind, ids, rows, inp, chans, stride):
        """one call of `dec` over rows [(stream id, packet or run)] under the stream ids `ids` -> one pending entry:
        ([(stream id, channels) per row], the rows' first packets [rows + 1], pcm, samples per row, samples, status)"""
        meta = [(sid, chans[r]) for r, (sid, _) in enumerate(rows)]
        if kind == "batch":
            pk, nb, gp, eo = inp
            pcm, samples, status = dec.synthesis_batch(ids, pk, nb, granulepos=gp, eos=eo,
                                                       out=self.out(len(ids), dec.channels, dec.row))
            return [(meta, list(range(len(rows) + 1)), pcm, samples, samples, status)]
        data, offs, gp, eo, gap = inp
        counts = [len(r) for _, r in rows]
        pcm, rs, samples, status = dec.synthesis_runs(ids, counts, data, offs, granulepos=gp, eos=eo, gap=gap,
                                                      out=self.out(len(ids), dec.channels, stride, sum(counts)))
        return [(meta, np.cumsum([0] + counts).tolist(), pcm, rs, samples, status)]

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

    def __init__(self, *a, compact=False, **kw):
        super().__init__(*a, **kw)
        self.dec, self.compact = {}, compact

    def play(self, script):
        """compact: every Decoder is sized to the streams its class is ever bound to and to the most rows a call gives
        it, and takes those streams under ids 0, 1, ... of its own (.local[class][stream id])"""
        of, self.local, self.need = {}, {}, {}
        for ev in script:
            if ev[0] == "bind":
                of.update(zip(ev[1], ev[2]))
                for s, c in zip(ev[1], ev[2]):
                    mine = self.local.setdefault(c, {})
                    mine.setdefault(s, len(mine))
            elif ev[0] in ("batch", "runs"):
                rows = {}
                for s, r in ev[1]:
                    rows[of[s]] = rows.get(of[s], 0) + (1 if ev[0] == "batch" else len(r))
                for c, n in rows.items():
                    self.need[c] = max(self.need.get(c, 1), n)
        return super().play(script)

    def ids(self, c, streams):
        return [self.local[c][s] for s in streams] if self.compact else list(streams)

    def add(self, c):
        S, cap = (len(self.local.get(c, [0])), self.need.get(c, 1)) if self.compact else (self.S, self.cap)
        self.dec[c] = self.v.Decoder(self.classes[c].ds, S, cap, halfrate=self.halfrate)

    def bind(self, ids, cs):
        for c in sorted(set(cs)):
            self.dec[c].restart_streams(self.ids(c, [s for s, k in zip(ids, cs) if k == c]))

    def call(self, kind, rows, inp):
        out = []
        for c in sorted({self.of[s] for s, _ in rows}):
            mine = [(s, r) for s, r in rows if self.of[s] == c]
            sub = (batch_inputs if kind == "batch" else runs_inputs)([r for _, r in mine], self.dev)
            stride = max([1] + [len(r) * self.row(c) for _, r in mine]) if kind == "runs" else None
            out += self.call_on(self.dec[c], kind, self.ids(c, [s for s, _ in mine]), mine, sub,
                                [self.classes[c].ch] * len(mine), stride)
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


def both(v, classes, script, S, cap, dev, halfrate=False, count=False, compact=False, **caps):
    """the script on a MixedDecoder and on the yardstick, compared -> the Mixed player (its .result, .blocks).
    compact: the yardstick's Decoders are sized to their own classes (PerClass.play)"""
    for k in classes:
        k.ds = v.DecodeSetup(k.headers)
    try:
        m = Mixed(v, classes, S, cap, dev, halfrate, count, **caps)
        got = m.play(script)
        want = PerClass(v, classes, S, cap, dev, halfrate, compact=compact).play(script)
        m.samples = same(got, want)
        assert m.samples > 0
    finally:
        for k in classes:
            k.ds.close()
    return m
