"""Device side of the encoder tests (torch and the library): the one per-block driver over Encoder.analysis_batch, the
replica check, and the from-PCM drivers over FrontEnd — drain / collect, the schedule runner DeviceRun, the rounds
runners with their delay fixtures.  The host side (oracle walk, schedule, comparers) is tests/encode_oracle.py.

A fixture defined here is imported by name into the test module that uses it (`# noqa: F401`)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import intake_cases as ic
from tests.encode_oracle import (compare_blobs, compare_block_call, compare_packets, compare_records, lockstep, record,
                                 records, setup_of, walk)
from tests.gpuutil import TwinLedger
from tests.signals import burst_signal, synth_signal


# ---- per block: Encoder.analysis_batch on oracle-carved blocks ---------------------------------------------------------
def check_replicas(held, Km, R, label):
    """held: [(name, tensor [R * Km * rows, ...], bool mask of its 32-bit words or None, rows per stream-block)].  Every
    row equals its signal's first row, bit for bit where the mask says so: one reduction and one host sync for the
    whole list.  -> rows held to their first copies"""
    held = [(name, t.contiguous().view(torch.int32).view(t.shape[0], -1), ok, rps) for name, t, ok, rps in held]
    flags, rows = [], 0
    for name, x, ok, rps in held:
        group = Km * rps
        assert x.shape[0] == R * group, (label, name, x.shape)
        ne = x.view(R, group, -1) != x[:group]
        if ok is not None:
            ne &= ok.view(R, group, -1)
        flags.append(ne.any())
        rows += x.shape[0] - group
    bad = torch.stack(flags).cpu().numpy()
    if bad.any():
        name, x, ok, rps = held[int(np.flatnonzero(bad)[0])]
        group = Km * rps
        ne = x.view(R, group, -1) != x[:group]
        if ok is not None:
            ne &= ok.view(R, group, -1)
        ne = ne.view(x.shape)
        rows_bad = torch.nonzero(ne.any(dim=1)).flatten()
        r = int(rows_bad[0])
        at = int(torch.nonzero(ne[r]).flatten()[0])
        raise AssertionError(
            f"{label}: identical input, different {name}: {rows_bad.numel()} of {x.shape[0]} rows differ from their signal's "
            f"first row; first: row {r} (lane {r % 64} of tile {r // 64}, stream-block row {r // rps}, channel {r % rps}) "
            f"against row {r % group}, first differing 32-bit word {at} of {x.shape[1]}: {int(x[r, at])} / "
            f"{int(x[r % group, at])}, {int(ne[r].sum())} words of the row differ; rows affected: {rows_bad[:12].tolist()}")
    return rows


def packet_words(packets, nbytes):
    """mask of every 32-bit word of a row that holds a byte of its packet"""
    return (torch.arange(packets.shape[1] // 4, device=packets.device)[None, :] * 4) < nbytes[:, None]


def run_lockstep(enc, cuda, streams, ch=None, float_stages=(), int_stages=(), res1_channels=(), R=1, stop="longest",
                 schedule=None, out_fill=None, poison=None, back_stream=None, on_call=None, label=""):
    """The one per-block driver: the calls of lockstep(streams, R, stop) (or of `schedule`, the same tuples) through
    enc.analysis_batch; the distinct blocks are uploaded and the replicas expanded on the device.  After every call the
    named stages are fetched; with R > 1 every row is held to its signal's first (check_replicas: the packets up to their
    lengths, whole rows where out_fill is given); the first copies go to the host and to compare_block_call /
    compare_packets.
    out_fill: the packet buffer is pre-filled with this byte (the lengths with -7) and every row must be zero past its
    packet.  poison: every workspace is filled with this byte before each call.  back_stream: the two-stream form, no host
    synchronisation between the calls; the packets are compared after one synchronize at the end (no stages).
    on_call(call) runs after the fetches and before the checks, with call.k, .mode, .present, .ids, .blks, .label,
    .packets, .nbytes, .got (stage -> device tensor) and .held (the list check_replicas gets: it may add to it).
    -> dict(modes = block types seen, calls, blocks = first-copy blocks compared, rows = rows held to their twins)"""
    stat = dict(modes=set(), calls=0, blocks=0, rows=0)
    pending = []
    for k, mode, present, ids, blks in (schedule if schedule is not None else lockstep(streams, R, stop)):
        Km, nsb = len(present), len(ids)
        where = f"{label} block {k} type {mode} signals {list(present)} ({nsb} stream-blocks)"
        if poison is not None:
            torch.cuda.synchronize()
            enc.debug_poison(-1, poison)
        pcm = torch.from_numpy(np.stack([b["pcm"] for b in blks])).to(cuda)
        if R > 1:
            pcm = pcm.index_select(0, torch.arange(nsb, device=cuda) % Km).contiguous()
        wflags = np.tile(np.array([b["lW"] | (b["nW"] << 1) for b in blks], np.uint8), R)
        out = None
        if out_fill is not None or back_stream is not None:
            out = (torch.full((nsb, enc.max_packet_bytes), out_fill or 0, dtype=torch.uint8, device=cuda),
                   torch.full((nsb,), -7, dtype=torch.int32, device=cuda))
        stat["modes"].add(mode)
        stat["calls"] += 1
        stat["blocks"] += Km
        if back_stream is not None:
            pending.append((where, blks, out))
            enc.analysis_batch(mode, ids, wflags, pcm, back_stream=back_stream, out=out)
            continue
        packets, nbytes = enc.analysis_batch(mode, ids, wflags, pcm, out=out)
        got = {name: enc.fetch(name) for name in tuple(float_stages) + tuple(int_stages)}
        held = [("packet lengths", nbytes, None, 1),
                ("packets", packets, None if out_fill is not None else packet_words(packets, nbytes), 1)] if R > 1 else []
        for name, t in got.items() if R > 1 else ():
            ok = None
            if name == "residue" and res1_channels:
                keep = torch.tensor([x not in res1_channels for x in range(ch)], device=cuda)
                ok = keep.repeat(nsb)[:, None].expand(-1, t.shape[1]).contiguous()
            held.append((name, t, ok, t.shape[0] // nsb))
        call = types.SimpleNamespace(k=k, mode=mode, present=present, ids=ids, blks=blks, label=where, packets=packets,
                                     nbytes=nbytes, got=got, held=held)
        if on_call is not None:
            on_call(call)
        if R > 1:
            stat["rows"] += check_replicas(held, Km, R, where)
        lead = {name: t[:Km * (t.shape[0] // nsb)].cpu().numpy() for name, t in got.items()}
        compare_block_call(lead, blks, ch, float_stages, int_stages, res1_channels, where)
        compare_packets(packets[:Km].cpu().numpy(), nbytes[:Km].cpu().numpy(), [b["packet"] for b in blks], where,
                        zero_tail=out_fill is not None)
    if pending:
        torch.cuda.synchronize()
        for where, blks, (packets, nbytes) in pending:
            compare_packets(packets.cpu().numpy(), nbytes.cpu().numpy(), [b["packet"] for b in blks], where)
    return stat


def fetch_blobs(enc, rows=None):
    """the fifteen packetblobs of the last call (the first `rows` rows), on the host: [(bytes, lengths)]"""
    out = []
    for kb in range(15):
        bp, bn = enc.fetch_blob(kb)
        out.append((bp[:rows].cpu().numpy(), bn[:rows].cpu().numpy()))
    return out


STAGES_F = ["mdct_raw", "logfft", "logmdct", "noise", "tone", "logmask", "mdct", "epeak", "npeak", "poste"]
STAGES_I = ["post_valid", "nonzero", "residue"]


def run_stages(oracle, cuda, ch, rate, q, makers, res1_channels=()):
    """The streams of `makers` [(name, make)] in one encoder, in lock step, end of stream included: every stage of
    STAGES_F / STAGES_I and the packet of every block, bit for bit.  `npeak` is compared as couple/quantise leaves it,
    which is where the oracle captures it.  -> counts of blocks, blocks with poste > 0, npeak entries of -1 in their
    channels, and batches that hold channel-blocks of both kinds"""
    import vorbis_aotuv_lancer_amd as v
    streams = [walk(oracle, ch, rate, q, pcm=make, key=("run_stages", name)) for name, make in makers]
    setup = v.Setup(ch, rate, q)
    enc = v.Encoder(setup, len(streams))
    count = dict(blocks=0, poste=0, minus1=0, mixed=0)

    def tally(call):
        ref = np.concatenate([b["poste"] for b in call.blks])
        count["blocks"] += len(call.blks)
        count["poste"] += sum(bool((b["poste"] > 0).any()) for b in call.blks)
        count["minus1"] += sum(int((b["npeak"][c] == -1).sum()) for b in call.blks for c in range(ch) if b["poste"][c] > 0)
        count["mixed"] += 0 < int((ref > 0).sum()) < len(ref)      # channel-blocks with and without, side by side in a tile

    run_lockstep(enc, cuda, streams, ch, STAGES_F, STAGES_I, res1_channels, on_call=tally, label=f"{ch}ch {rate} q{q:g}")
    enc.close()
    setup.close()
    print(f"{ch}ch {rate} q{q:g}: {count['blocks']} blocks compared, {count['poste']} with poste > 0, "
          f"{count['minus1']} npeak entries of -1 in their channels with poste > 0, {count['mixed']} batches with both kinds of channel-block")
    return count


def managed_blobs(oracle, cuda, bitrate, makers):
    """2ch 44100 managed, the streams of `makers` in one encoder: poste, all fifteen packetblobs (the chosen one up to
    where the oracle cut it), the bitrate manager's choice and the delivered packet of every block
    -> (blocks compared, blocks with poste > 0, packets cut)"""
    import vorbis_aotuv_lancer_amd as v
    ch, rate = 2, 44100
    streams = [walk(oracle, ch, rate, bitrate=bitrate, pcm=make, key=("run_stages", name)) for name, make in makers]
    setup = v.Setup(ch, rate, bitrate=bitrate)
    enc = v.Encoder(setup, len(streams))
    n = dict(blocks=0, poste=0, cut=0)

    def blobs(call):
        n["cut"] += compare_blobs(fetch_blobs(enc), enc.fetch("choice").cpu().numpy(), call.blks, call.label, cut=True)
        n["blocks"] += len(call.blks)
        n["poste"] += sum(bool((b["poste"] > 0).any()) for b in call.blks)

    run_lockstep(enc, cuda, streams, ch, ("poste",), on_call=blobs, label=f"2ch 44100 b{bitrate}")
    enc.close()
    setup.close()
    print(f"2ch 44100 b{bitrate}: {n['blocks']} blocks compared with all blobs, {n['poste']} with poste > 0, {n['cut']} packets cut")
    return n["blocks"], n["poste"], n["cut"]


# ---- from PCM: FrontEnd rounds -------------------------------------------------------------------------------------------
def split_dump(d):
    out, at = [], 0
    while at < len(d):
        n = int.from_bytes(d[at:at + 4], "little")
        out.append(d[at + 4:at + 4 + n])
        at += 4 + n
    return out


def probe_pcm(oracle, ch, rate, secs):
    total = rate * secs
    n = ((total + 1023) // 1024) * 1024          # the probe driver writes whole 1024-sample chunks
    out = np.empty((ch, n), np.float32)
    oracle.lib.orc_probe_signal.argtypes = [C.c_int, C.c_long, C.c_long, C.c_void_p]
    oracle.lib.orc_probe_signal(ch, rate, n, out.ctypes.data)
    return out


def collect(sink, info, packets, nbytes):
    packets = packets.cpu().numpy()
    nbytes = nbytes.cpu().numpy()
    for k, pi in enumerate(info):
        assert nbytes[k] >= 0, "packet buffer overflow"
        sink[int(pi["stream"])].append(record(pi, bytes(packets[k, :nbytes[k]])))


def drain(fe, sink, max_rounds=None, multi=False):
    """rounds until no stream has a block (or, with max_rounds, until that many rounds ran and no buffer
    is more than half full); sink[stream] collects (info fields, packet bytes).  multi: through
    vbm_frontend_encode_rounds (several rounds per call, joined at the end)"""
    if multi == "lazy":
        # lazy joins: the outputs of a call are complete once the next call has been enqueued (or after join)
        held = getattr(fe, "_held", None)
        while True:
            out = fe.encode_rounds(min_rounds=max_rounds or 64, max_rounds=4 if max_rounds is None else 16, lazy=True)
            if held is not None:
                collect(sink, held[0].copy(), held[1], held[2])
            held = (out[0], out[1], out[2])
            if not out[3] or max_rounds is not None:
                break
        fe._held = held
        return
    if multi:
        while True:
            info, packets, nbytes, counts = fe.encode_rounds(min_rounds=max_rounds or 64, max_rounds=4 if max_rounds is None else 16)
            collect(sink, info, packets, nbytes)
            if not counts or max_rounds is not None:
                return
    rounds = 0
    while True:
        if max_rounds is not None and rounds >= max_rounds and fe.max_buffered + 1024 <= fe.capacity // 2:
            return
        rounds += 1
        info, packets, nbytes = fe.encode_round()
        if len(info) == 0:
            return
        collect(sink, info, packets, nbytes)


def flush_held(fe, sink):
    """the outputs a lazy drain still holds back"""
    if getattr(fe, "_held", None) is not None:
        fe.join()
        collect(sink, fe._held[0].copy(), fe._held[1], fe._held[2])
        fe._held = None


def collect_device(sink, fe, out):
    """outputs of one encode_rounds_device call (device tensors) -> sink[stream]"""
    import vorbis_aotuv_lancer_amd as v
    info, packets, nbytes, counts = out
    nb = nbytes.cpu().numpy()
    live = np.flatnonzero(nb != -2)
    if len(live) == 0:
        return 0
    rec = info.cpu().numpy().view(np.dtype(v.PacketInfo))[:, 0]
    pk = packets[torch.from_numpy(live).to(packets.device)].cpu().numpy()
    for j, k in enumerate(live):
        pi = rec[k]
        assert nb[k] >= 0, "packet buffer overflow"
        assert pi["stream"] >= 0
        sink[int(pi["stream"])].append(record(pi, bytes(pk[j, :nb[k]])))
    # the counts are the live lanes per block type, and every region is filled from its start
    c = counts.cpu().numpy()
    assert int(c.sum()) == len(live)
    return len(live)


def write_and_drain(fe, cuda, sigs, got, chunk=1024, finish=True, **drain_args):
    """every stream's signal `chunk` samples per write, drained after every write (drain_args: as drain), then, with
    finish, drained once more, ended and drained"""
    allp = torch.from_numpy(np.stack(sigs)).to(cuda)
    for at in range(0, allp.shape[2], chunk):
        fe.write(allp[:, :, at:at + chunk].contiguous())
        drain(fe, got, **drain_args)
    if finish:
        # vorbis_analysis_wrote(vd, 0) fits its end-of-stream LPC to what the buffer holds at that moment
        # (lib/block.c:531-541), so, like the reference application loop, drain before finishing
        flush_held(fe, got)
        drain(fe, got)
        fe.finish()
        drain(fe, got)


def frontend_vs_oracle(oracle, cuda, ch, rate, q, NS, seconds, need_modes=(0, 1, 2, 3), max_rounds=None, bitrate=None,
                       sigs=None, multi=False):
    import vorbis_aotuv_lancer_amd as v
    nsamp = int(seconds * rate) // 1024 * 1024
    if sigs is None:
        sigs = [synth_signal(ch, rate, nsamp, seed=500 + s, level=1.0 if s % 3 else 0.05) for s in range(NS)]
    # oracle: same write pattern (1024 at a time, drain after every write, then end of stream)
    want = [records(walk(oracle, ch, rate, q, bitrate, sigs[s][:, :nsamp], capture=False)) for s in range(NS)]
    enc = v.Encoder(v.Setup(ch, rate, q, bitrate=bitrate), NS)
    fe = v.FrontEnd(enc)
    got = [[] for _ in range(NS)]
    write_and_drain(fe, cuda, [x[:, :nsamp] for x in sigs], got, max_rounds=max_rounds, multi=multi)
    modes = set()
    for s in range(NS):
        compare_records(got[s], want[s], f"stream {s}")
        modes |= {m[3] for m, _ in got[s]}
    assert modes >= set(need_modes), modes


# ---- from PCM: a schedule of writes, drains, ends and restarts (tests/intake_cases.py) --------------------------------------
_wanted = {}


def osetup(oracle, cls):
    return setup_of(oracle, *cls)


def wanted(oracle, cls, key, signals, schedule):
    """the oracle's sequences for a (class, case): computed once, shared by the tests that replay the case"""
    if (cls, key) not in _wanted:
        _wanted[(cls, key)] = ic.oracle_run(oracle, osetup(oracle, cls), signals, schedule)
    return _wanted[(cls, key)]


class DeviceRun:
    """One FrontEnd driven through a schedule.  how: "write" (FrontEnd.write: every stream, one size), "streams"
    (write_streams, one call per distinct size of a step) or "strided" (write_streams_strided from a device arena:
    by slot, channel stride larger than any write, base one float off 16-byte alignment).
    rounds: None = host-built rounds until nothing is left; n = every drain runs n device-built rounds first, and where
    an end, a restart or nothing follows, host-built rounds then carve what is left (the end-of-stream fit wants the
    buffer drained).  device_count[s] / device_eos[s]: blocks / e_o_s blocks of slot s that device-built rounds carved."""
    ARENA = 4100

    def __init__(self, cuda, cls, nstreams, how, rounds=None):
        import vorbis_aotuv_lancer_amd as v
        self.v, self.cuda, self.how, self.rounds = v, cuda, how, rounds
        self.setup = v.Setup(*cls)
        self.S, self.ch = nstreams, cls[0]
        lanes = v.lib.vbm_device_round_lanes(self.setup._h, nstreams) if rounds else None
        self.enc = v.Encoder(self.setup, nstreams, max_batch=lanes)
        self.fe = v.FrontEnd(self.enc)
        self.got = [[] for _ in range(nstreams)]
        self.done = {s: [] for s in range(nstreams)}     # finished logical streams of a slot
        self.at = [0] * nstreams
        self.gen = [0] * nstreams
        self.device_blocks = 0
        self.device_count = [0] * nstreams
        self.device_eos = [0] * nstreams
        if how == "strided":
            self.flat = torch.zeros(1 + nstreams * self.ch * self.ARENA, dtype=torch.float32, device=cuda)
            self.arena = self.flat[1:].view(nstreams, self.ch, self.ARENA)
            assert self.arena.data_ptr() % 16 == 4

    def signal(self, signals, s):
        sig = signals[s]
        return sig[self.gen[s]] if isinstance(sig, (list, tuple)) else sig

    def write(self, signals, sizes):
        pcs = {}
        for s, n in sizes.items():
            sig = self.signal(signals, s)
            assert n > 0 and self.at[s] + n <= sig.shape[1]
            pcs[s] = sig[:, self.at[s]:self.at[s] + n]
            self.at[s] += n
        if self.how == "write":
            n = next(iter(sizes.values()))
            assert sorted(sizes) == list(range(self.S)) and all(m == n for m in sizes.values())
            self.fe.write(torch.from_numpy(np.stack([pcs[s] for s in range(self.S)])).to(self.cuda).contiguous())
            return
        for n in sorted(set(sizes.values())):
            ids = [s for s in sorted(sizes) if sizes[s] == n]
            if self.how == "streams":
                self.fe.write_streams(ids, torch.from_numpy(np.stack([pcs[s] for s in ids])).to(self.cuda).contiguous())
            else:
                assert n < self.ARENA
                for s in ids:
                    self.arena[s, :, :n] = torch.from_numpy(np.ascontiguousarray(pcs[s])).to(self.cuda)
                torch.cuda.synchronize()
                self.fe.write_streams_strided(ids, self.arena, n, self.ch * self.ARENA, self.ARENA, by_slot=True)

    def run(self, signals, schedule):
        for k, step in enumerate(schedule):
            if step[0] == "write":
                self.write(signals, step[1])
            elif step[0] == "drain":
                ahead = schedule[k + 1][0] if k + 1 < len(schedule) else "finish"
                if self.rounds:
                    before = [len(g) for g in self.got]
                    out = self.fe.encode_rounds_device(nrounds=self.rounds)
                    self.device_blocks += collect_device(self.got, self.fe, out)
                    for s in range(self.S):
                        self.device_count[s] += len(self.got[s]) - before[s]
                        self.device_eos[s] += sum(m[4] for m, _ in self.got[s][before[s]:])
                if not self.rounds or ahead != "write":
                    drain(self.fe, self.got)
            elif step[0] == "finish":
                self.fe.finish(step[1])
            elif step[0] == "restart":
                for s in step[1]:
                    self.done[s].append(self.got[s])
                    self.got[s] = []
                    self.at[s] = 0
                    self.gen[s] += 1
                self.fe.restart_streams(step[1])
        if self.rounds:
            self.fe.device_stats()
            assert self.fe.refused_writes == 0
        return {s: self.done[s] + [self.got[s]] for s in range(self.S)}

    def close(self):
        self.fe.close()
        self.enc.close()


def compare_slots(got, want, label=""):
    """{slot: [records of its first logical stream, of its second, ...]} of DeviceRun.run against oracle_run's"""
    for s in sorted(want):
        assert len(got[s]) == len(want[s]), (label, s)
        for g, (a, b) in enumerate(zip(got[s], want[s])):
            compare_records(a, b, f"{label} stream {s}.{g}")


def need_types(cls, want):
    # two block sizes: long and short blocks both occur; one size (mono 8 kHz): types 0 and 1
    types = {m[3] for seqs in want.values() for seq in seqs for m, _ in seq}
    if cls == ic.CLASSES[2]:
        assert types >= {0, 1}, types
    else:
        assert types & {0, 1} and 3 in types, types


# ---- rounds at size: 2048 streams, 8 twin signals, internal HIP streams held up -------------------------------------------
CH, RATE, Q = 2, 44100, 0.5
S, K = 2048, 8                  # 256 twins per signal: batches of 256 .. 2048 blocks (small and "big" ones, >= 1024)
DELAY_US = 3000                 # longer than any kernel of a batch of this size
MANAGED = (144000, 128000, 112000)     # vorbis_encode_init(max, nominal, min): the bitrate manager's reservoirs are carried state

# csrc/vbm_internal.h, enum vbm_delay_point
POINTS = {"job_big": 0, "job_small": 1, "job_state": 2, "job_back": 3, "job_out": 4, "fe_fork": 5, "fe_shift": 6,
          "dev_big_front": 7, "dev_big_back": 8, "dev_small_front": 9, "dev_small_back": 10, "dev_plan": 11,
          "batch_front": 12, "batch_back": 13, "fe_write": 14, "dev_out": 15, "dev_big_transforms": 16,
          "dev_small_transforms": 17}
_signals = {}


@pytest.fixture
def delay():
    """delay(*points): a spin kernel of DELAY_US in front of the work behind every named point, until the test ends"""
    import vorbis_aotuv_lancer_amd as v

    def set_points(*names):
        mask = 0
        for n in names:
            mask |= 1 << POINTS[n]
        assert v.lib.vbm_debug_set_delay(mask, DELAY_US if mask else 0) == 0
    yield set_points
    v.lib.vbm_debug_set_delay(0, 0)


def signals(nchunks, period):
    key = (nchunks, period)
    if key not in _signals:
        _signals[key] = [burst_signal(CH, RATE, nchunks * 1024, seed=70 + k, period=period, level=1.0 if k % 3 else 0.05)
                         for k in range(K)]
    return _signals[key]


def make_setup(v, bitrate):
    return v.Setup(CH, RATE, bitrate=bitrate) if bitrate else v.Setup(CH, RATE, Q)


def oracle_want(oracle, nchunks, period, bitrate=None):
    """per signal the oracle's packets, end of stream included: computed once"""
    return [[b["packet"] for b in walk(oracle, CH, RATE, None if bitrate else Q, bitrate, sig, capture=False,
                                       keep=("packet",), key=("rounds", k, period))]
            for k, sig in enumerate(signals(nchunks, period))]


def drain_host(fe, led, label):
    while True:
        info, packets, nbytes = fe.encode_round()
        if len(info) == 0:
            return
        led.add_host_round(info, packets, nbytes, label)


def run_host_rounds(cuda, nchunks, period, poison=False, multi=False, bitrate=None):
    import vorbis_aotuv_lancer_amd as v
    base = torch.from_numpy(np.stack(signals(nchunks, period))).to(cuda)
    enc = v.Encoder(make_setup(v, bitrate), S)
    fe = v.FrontEnd(enc)
    led = TwinLedger(S, K, cuda)
    for c in range(nchunks):
        if poison:
            enc.debug_poison(-1, 0xFF)
            fe.debug_poison(0xFF)
        fe.write(base[:, :, c * 1024:(c + 1) * 1024].repeat(S // K, 1, 1).contiguous())
        if multi:
            while True:
                info, packets, nbytes, counts = fe.encode_rounds(min_rounds=64, max_rounds=4)
                if not counts:
                    break
                led.add_host_round(info.copy(), packets, nbytes, f"write {c}")
        else:
            drain_host(fe, led, f"write {c}")
    fe.finish()
    drain_host(fe, led, "end of stream")
    led.finish("host-built rounds")
    fe.close()
    enc.close()
    return led


def run_device_rounds(cuda, monkeypatch, nchunks, period, poison=False, lazy=2, bitrate=None, workspaces="4"):
    import vorbis_aotuv_lancer_amd as v
    monkeypatch.setenv("VBM_WORKSPACES", workspaces)
    base = torch.from_numpy(np.stack(signals(nchunks, period))).to(cuda)
    setup = make_setup(v, bitrate)
    enc = v.Encoder(setup, S, max_batch=v.lib.vbm_device_round_lanes(setup._h, S))
    fe = v.FrontEnd(enc)
    led = TwinLedger(S, K, cuda)
    consumer = torch.cuda.Stream(device=cuda)
    for c in range(nchunks):
        if poison:
            fe.join()
            enc.debug_poison(-1, 0xFF)
            fe.debug_poison(0xFF)
        fe.write(base[:, :, c * 1024:(c + 1) * 1024].repeat(S // K, 1, 1).contiguous())
        info, packets, nbytes, counts = fe.encode_rounds_device(nrounds=2, lazy=lazy)
        fe.join(consumer)
        with torch.cuda.stream(consumer):
            led.add_device_rounds(info, packets, nbytes, f"write {c}")
        consumer.synchronize()
    fe.device_stats()
    assert fe.refused_writes == 0
    torch.cuda.synchronize()
    drain_host(fe, led, "drain")
    fe.finish()
    drain_host(fe, led, "end of stream")
    led.finish("device-built rounds")
    fe.close()
    enc.close()
    return led


def check_oracle(led, oracle, nchunks, period, bitrate=None):
    want = oracle_want(oracle, nchunks, period, bitrate)
    for k in range(K):
        assert led.lead_packets(k) == want[k], f"signal {k}: packets differ from the oracle"
    assert led.modes[0] + led.modes[1] > 0 and led.modes[2] > 0 and led.modes[3] > 0, led.modes   # all block types ran
