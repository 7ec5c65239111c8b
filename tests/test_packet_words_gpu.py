"""Packet rows, whole: what the caller's packet buffer holds after a VBR batch.  k_packets_out (csrc/pack_kernels.hip) takes a
packet's own words from the word-major tile, writes zeros for the rest of the row without reading it, skips the loads of
a 64-row tile that lies above the longest packet of its 64 lanes, and copies the lengths.

One rule for every case: the destination is pre-filled with 0xA5 and every workspace is poisoned with 0xFF before the
work; then row[:nb] is the oracle's packet and row[nb:] is zero up to max_packet_bytes.  Where a case holds replicas of a
signal, the replicas' whole rows equal the first copy's on the device and the first copies go to the host.

The cases also cover what packet assembly does in front of it (k_res_offsets / k_res_emit: phrase codewords, several
residue submaps, several coded vectors, both slice forms), with tiles that held other packets or poison before.

Shipped mode packs by residue shape (csrc/setup_host.cpp tables): every pack's phrase book has dimension 2 except
mode_6ch_48000_q1 (dimension 1, res2 over five channels); the 6-channel packs have two residue submaps (res2 of five
channels, res1 of the LFE); the 3/4/5/7/8-channel packs are uncoupled res1 (one coded vector per nonzero channel)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import encode_calls as ec
from tests import orc
from tests.encode_oracle import compare_packets, walk
from tests.signals import burst_signal, synth_signal

pytestmark = pytest.mark.gpu

FILL, POISON = 0xA5, 0xFF


def oracle_blocks(oracle, ch, rate, q, name, pcm):
    """the oracle's blocks of one signal (1024 samples per write, end of stream declared): computed once"""
    assert pcm.shape[1] % 1024 == 0
    return walk(oracle, ch, rate, q, pcm=pcm, keep=("pcm", "lW", "nW", "N", "block_mode", "packet"), key=("packet_words", name))


def silence(ch, n):
    return np.zeros((ch, n), np.float32)


def loud_noise(ch, n, seed):
    return (0.98 * np.random.default_rng(seed).uniform(-1, 1, (ch, n))).astype(np.float32)


def filled(shape, dtype, value, dev):
    return torch.full(shape, value, dtype=dtype, device=dev)


def run_lockstep(cuda, enc, streams, R, label):
    """K oracle streams replicated R times through Encoder.analysis_batch (tests/encode_calls.py, run_lockstep): the
    destination pre-filled, every workspace poisoned before every call, whole rows compared; -> block types seen"""
    return ec.run_lockstep(enc, cuda, streams, R=R, out_fill=FILL, poison=POISON, label=label)["modes"]


# ---- per-block path: two lane tiles, short packets over long ones ---------------------------------------------------------
NWS = 2


def stale_case(oracle):
    """2ch 44100 q0.5: digital silence, synth_signal and near-full-scale noise -> (the three signals' blocks, per signal
    the index of its first long block that 2 * NWS - 1 more long blocks follow).  The streams open with different block
    types (silence has no impulse block), so each is taken through its opening blocks alone and the 70-stream calls
    begin at these indices."""
    ch, rate, q, n = 2, 44100, 0.5, 16 * 1024
    sigs = [("silence", silence(ch, n)), ("synth", synth_signal(ch, rate, n, seed=21, level=0.6)), ("noise", loud_noise(ch, n, 22))]
    streams = [oracle_blocks(oracle, ch, rate, q, name, pcm) for name, pcm in sigs]
    starts = []
    for blks in streams:
        modes = [b["block_mode"] for b in blks]
        starts.append(next(k for k in range(len(modes)) if modes[k:k + 2 * NWS] == [3] * (2 * NWS)))
    return streams, starts


def test_stale_case_has_short_and_long_packets(oracle):
    """the condition of the per-block case, on the CPU: among the packets of its 70-stream calls some are shorter than 64
    bytes and some longer than 512, so two 256-byte row-tile boundaries lie between the short and the long packets of a
    tile; every call has packets below 64 bytes beside packets above 256"""
    streams, starts = stale_case(oracle)
    per_call = [[len(s[at + k]["packet"]) for s, at in zip(streams, starts)] for k in range(2 * NWS)]
    assert min(min(c) for c in per_call) < 64 and max(max(c) for c in per_call) > 512, per_call
    assert all(min(c) < 64 and max(c) > 256 for c in per_call), per_call


def test_per_block_two_tiles_short_packets_over_long_ones(oracle, cuda, monkeypatch):
    """70 streams: tile 0 mixes the three signals, tile 1 has six lanes, all silent.  2 * nws calls of long blocks; from one
    use of a workspace to the next every lane of tile 0 changes its signal, so long packets lie stale under short ones.
    The workspaces are poisoned before the first use of each; the second use runs over what the first left."""
    import vorbis_aotuv_lancer_amd as v
    monkeypatch.setenv("VBM_WORKSPACES", str(NWS))
    streams, starts = stale_case(oracle)
    S = 70
    sig_of = np.array([s % 3 for s in range(64)] + [0] * 6)         # stream -> signal; streams 64..69 silent
    setup = v.Setup(2, 44100, 0.5)
    enc = v.Encoder(setup, S)

    def call(ids, k_of, label):
        blks = [streams[sig_of[s]][k_of[sig_of[s]]] for s in ids]
        mode = blks[0]["block_mode"]
        assert all(b["block_mode"] == mode for b in blks)
        pcm = torch.from_numpy(np.stack([b["pcm"] for b in blks])).to(cuda).contiguous()
        wflags = np.array([b["lW"] | (b["nW"] << 1) for b in blks], np.uint8)
        out = (filled((len(ids), enc.max_packet_bytes), torch.uint8, FILL, cuda), filled((len(ids),), torch.int32, -7, cuda))
        packets, nbytes = enc.analysis_batch(mode, np.asarray(ids, np.int32), wflags, pcm, out=out)
        compare_packets(packets.cpu().numpy(), nbytes.cpu().numpy(), [b["packet"] for b in blks], label, zero_tail=True)

    enc.debug_poison(-1, POISON)
    for m in range(3):                                               # the opening blocks, a signal's streams per call
        for k in range(starts[m]):
            call(np.flatnonzero(sig_of == m), {m: k}, f"opening block {k} of signal {m}")
    torch.cuda.synchronize()
    enc.debug_poison(-1, POISON)
    before = {}
    for k in range(2 * NWS):
        shift = (k // NWS) % 2                                       # lane i of tile 0 holds stream (i + shift) % 64
        ids = np.concatenate([(np.arange(64) + shift) % 64, np.arange(64, 70)])
        if k >= NWS:                                                 # the lane's packet one use of the workspace ago: another signal's
            assert sum(sig_of[ids[i]] != sig_of[before[k % NWS][i]] for i in range(64)) >= 63
        before[k % NWS] = ids
        call(ids, {m: starts[m] + k for m in range(3)}, f"call {k}")
    enc.close()
    setup.close()


# ---- device-built rounds: counts far below the launch bounds -------------------------------------------------------------
def test_device_built_rounds_eight_streams(oracle, cuda, monkeypatch):
    """8 streams with bursts (the signals and oracle packets of the rounds runners, tests/encode_calls.py), rounds built on the device:
    every block type's region is launched for its bound (thousands of lanes) and holds a handful of blocks"""
    import vorbis_aotuv_lancer_amd as v
    nchunks, period, S = 18, 12000, ec.K
    monkeypatch.setenv("VBM_WORKSPACES", "4")
    want = ec.oracle_want(oracle, nchunks, period)
    base = torch.from_numpy(np.stack(ec.signals(nchunks, period))).to(cuda)
    setup = v.Setup(ec.CH, ec.RATE, ec.Q)
    lanes = v.lib.vbm_device_round_lanes(setup._h, S)
    enc = v.Encoder(setup, S, max_batch=lanes)
    fe = v.FrontEnd(enc)
    nrounds = 2
    n = nrounds * lanes
    got = [dict() for _ in range(S)]                                 # packetno -> packet
    modes = np.zeros(4, np.int64)

    def collect(info, packets, nbytes, label):
        live = torch.nonzero(nbytes != -2).flatten()
        if live.numel() == 0:
            return
        rec = info.view(torch.int32)[live].cpu().numpy() if info.dtype == torch.uint8 else None
        pk, nb = packets[live].cpu().numpy(), nbytes[live].cpu().numpy()
        pno = info.view(torch.int64)[live][:, 4].cpu().numpy()
        for i in range(len(nb)):
            s, m = int(rec[i, 0]), int(rec[i, 1])
            assert 0 <= s < S and nb[i] >= 0, (label, s, int(nb[i]))
            assert not pk[i, nb[i]:].any(), (label, "row not zero past the packet", "stream", s, "type", m, "length", int(nb[i]))
            assert int(pno[i]) not in got[s], (label, "packet twice", s, int(pno[i]))
            got[s][int(pno[i])] = bytes(pk[i, :nb[i]])
            modes[m] += 1

    for c in range(nchunks):
        fe.join()
        torch.cuda.synchronize()
        enc.debug_poison(-1, POISON)
        fe.debug_poison(POISON)
        info = torch.zeros((n, C.sizeof(v.encoder.PacketInfo)), dtype=torch.uint8, device=cuda)
        packets = filled((n, enc.max_packet_bytes), torch.uint8, FILL, cuda)
        nbytes = filled((n,), torch.int32, -2, cuda)
        counts = torch.zeros((nrounds, 4), dtype=torch.int32, device=cuda)
        fe.write(base[:, :, c * 1024:(c + 1) * 1024].contiguous())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        v.encoder.check(v.lib.vbm_frontend_encode_rounds_device(fe._h, nrounds, packets.data_ptr(), nbytes.data_ptr(),
                                                                info.data_ptr(), counts.data_ptr(), 0, st),
                        "vbm_frontend_encode_rounds_device")
        fe.join()
        torch.cuda.synchronize()
        collect(info, packets, nbytes, f"write {c}")
    fe.device_stats()
    assert fe.refused_writes == 0

    def drain(label):
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                return
            pk, nb = packets.cpu().numpy(), nbytes.cpu().numpy()
            for i in range(len(info)):
                s = int(info["stream"][i])
                assert not pk[i, nb[i]:].any(), (label, "row not zero past the packet", s)
                got[s][int(info["packetno"][i])] = bytes(pk[i, :nb[i]])
                modes[int(info["block_mode"][i])] += 1

    drain("drain")
    fe.finish()
    drain("end of stream")
    for k in range(S):
        assert [got[k][pn] for pn in sorted(got[k])] == want[k], f"signal {k}: packets differ from the oracle"
    assert modes[0] + modes[1] > 0 and modes[2] > 0 and modes[3] > 0, modes
    fe.close()
    enc.close()
    setup.close()


# ---- submap and vector shapes ---------------------------------------------------------------------------------------------
SHAPES = [
    # two residue submaps (res2 of five channels + res1 of the LFE), phrase pairs
    ("6ch_48000_q0.5", 6, 48000, 0.5),
    # uncoupled: one coded vector per nonzero channel (used > 1), the generic phrase walk
    ("3ch_44100_q0.5", 3, 44100, 0.5),
    # the one shipped pack whose phrase book has dimension 1 (a phrase codeword per partition), two submaps
    ("6ch_48000_q1", 6, 48000, 1.0),
]


def one_live_channel(ch, rate, n, seed):
    """channel 1 only: in an uncoupled class the coded vectors are then fewer than the channels"""
    x = synth_signal(ch, rate, n, seed=seed)
    x[0] = 0
    x[2:] = 0
    return x


@pytest.mark.parametrize("name,ch,rate,q", SHAPES, ids=[s[0] for s in SHAPES])
def test_submap_and_vector_shapes(oracle, cuda, name, ch, rate, q):
    import vorbis_aotuv_lancer_amd as v
    d = v.tables.pack(orc.mode_pack_name(ch, rate, q))
    maps = [m for m in range(int(d["info/counts"][1]))]
    submaps = {int(d[f"map/{m}/submaps"][0]) for m in maps}
    pdims = {int(d[f"book/{int(d['residue/%d/head' % int(d[f'map/{m}/residuesubmap'][i])][6])}/head"][0])
             for m in maps for i in range(int(d[f"map/{m}/submaps"][0]))}
    if name.startswith("6ch"):
        assert submaps == {2}
    if name == "3ch_44100_q0.5":
        assert all(int(d[f"map/{m}/coupling_steps"][0]) == 0 for m in maps)
    assert pdims == ({1, 2} if name == "6ch_48000_q1" else {2}), pdims
    n = 12 * 1024
    sigs = [("burst", burst_signal(ch, rate, n, seed=31, period=5000)), ("synth", synth_signal(ch, rate, n, seed=32, level=0.5)),
            ("one_live", one_live_channel(ch, rate, n, 33)), ("silence", silence(ch, n))]
    streams = [oracle_blocks(oracle, ch, rate, q, nm, pcm) for nm, pcm in sigs]
    setup = v.Setup(ch, rate, q)
    R = 3
    enc = v.Encoder(setup, len(streams) * R)
    seen = run_lockstep(cuda, enc, streams, R, name)
    assert seen & {0, 1} and 3 in seen, seen          # short and long blocks
    enc.close()
    setup.close()


# ---- both slice forms of k_res_vq / k_res_emit ----------------------------------------------------------------------------
def slice_bounds(partvals, nsb):
    """first partitions of the slices a batch of nsb stream-blocks is cut into (csrc/pack_kernels.hip, vbm_launch_pack)"""
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd.encoder import COARSE_RESIDUE_SLICES
    most = 32 if v.batch_variants(3, 1024, 2, nsb) & COARSE_RESIDUE_SLICES else 256
    nchunks = max(1, min(partvals, most))
    return nchunks, [partvals * y // nchunks for y in range(nchunks)]


def smallest_coarse_nsb():
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd.encoder import COARSE_RESIDUE_SLICES
    lo, hi = 1, 2
    while not v.batch_variants(3, 1024, 2, hi) & COARSE_RESIDUE_SLICES:
        lo, hi = hi, hi * 2
        assert hi < 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if v.batch_variants(3, 1024, 2, mid) & COARSE_RESIDUE_SLICES else (mid, hi)
    return hi


@pytest.mark.parametrize("form", ["fine", "coarse"])
def test_both_slice_forms_cut_a_phrase_pair(oracle, cuda, form):
    """2ch 44100 q0.5 (phrase pairs): a batch below the limit of vbm_debug_batch_variants has a slice per partition, one
    at the limit at most 32 slices; in both a slice begins at an odd partition, inside a phrase pair, in the long blocks:
    the pair's two runs are then OR-ed into the packet by different slices, behind the pair's phrase codeword."""
    import vorbis_aotuv_lancer_amd as v
    ch, rate, q = 2, 44100, 0.5
    d = v.tables.pack(orc.mode_pack_name(ch, rate, q))
    n = 8 * 1024
    sigs = [("burst8", burst_signal(ch, rate, n, seed=41, period=5000)), ("noise8", loud_noise(ch, n, 42)),
            ("synth8", synth_signal(ch, rate, n, seed=43, level=0.5))]
    streams = [oracle_blocks(oracle, ch, rate, q, nm, pcm) for nm, pcm in sigs]
    K = len(streams)
    limit = smallest_coarse_nsb()
    R = (limit + K - 1) // K if form == "coarse" else 30        # fine: 90 stream-blocks, two tiles, the second partial
    if form == "coarse":
        while (R * K) % 64 == 0:
            R += 1
    for m in range(int(d["info/counts"][1])):
        head = d[f"residue/{int(d[f'map/{m}/residuesubmap'][0])}/head"]
        partvals = (int(head[2]) - int(head[1])) // int(head[3])
        nchunks, bounds = slice_bounds(partvals, R * K)
        assert nchunks == (partvals if form == "fine" else min(partvals, 32)), (form, nchunks, partvals)
        if m == 1:
            assert any(b % 2 for b in bounds), (form, partvals, bounds)
    setup = v.Setup(ch, rate, q)
    enc = v.Encoder(setup, K * R)
    seen = run_lockstep(cuda, enc, streams, R, f"{form} slices")
    assert seen & {0, 1} and 3 in seen, seen
    enc.close()
    setup.close()
