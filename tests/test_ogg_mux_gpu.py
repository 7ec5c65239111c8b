"""vbm_ogg_mux_packets on the device: equal to its host twin byte for byte (bytes, offsets, status) on the schedules
of the CPU file at 1024 streams, and end to end from PCM — header pages + muxed bytes of every stream equal write_ogg
of the stream's packets, and decode back to the stream's sample count."""
import numpy as np
import pytest
import torch

from tests import oggmux_cases as oc
from tests.signals import burst_signal, synth_signal

pytestmark = pytest.mark.gpu


def both(mux, info, packets, nbytes, flush, what):
    """one call through the device and through the twin; -> the call's bytes (numpy), offsets"""
    import vorbis_aotuv_lancer_amd as v  # noqa: F401
    dev = mux.device
    out, offsets, status = mux.mux(info, torch.from_numpy(packets).to(dev), torch.from_numpy(nbytes).to(dev), flush)
    hout, hoffsets, hstatus = mux.mux_host(info, packets, nbytes, flush)
    offsets, status = offsets.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(status, hstatus), f"{what}: status {np.flatnonzero(status != hstatus)[:8]}"
    assert np.array_equal(offsets, hoffsets), f"{what}: offsets differ first at stream {np.flatnonzero(offsets != hoffsets)[:4]}"
    got = out[:int(offsets[-1])].cpu().numpy()
    if not np.array_equal(got, hout):
        at = int(np.flatnonzero(got != hout)[0])
        s = int(np.searchsorted(offsets, at, side="right") - 1)
        raise AssertionError(f"{what}: byte {at} differs (stream {s}, byte {at - offsets[s]} of its {offsets[s + 1] - offsets[s]})")
    return got, offsets, status


def test_device_equals_host_twin_on_the_directed_cases(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    n, M, R = 1024, 8192, 16
    rng = np.random.default_rng(77)
    scheds = []
    for s in range(n):                                     # a different schedule per stream: kind by s % 7, own sizes / delay
        scheds.append(oc.directed(rng, M, R)[s % 7])
    case = oc.Case(scheds, M, seed=21, flush_at=(5, 11), delays=[int(rng.integers(0, 6)) for _ in range(n)])
    mux = v.OggMux(setup, n, M, max_rows_per_stream=R)
    hdr = mux.start()
    w = oc.Writer(setup, n)
    for s in range(n):
        assert hdr[s] == w.start(s, s)
    seen_status = set()
    pages = 0
    for t, (restarts, rows, flush, hole_rng) in enumerate(case.steps()):
        if restarts:
            hdr = mux.start([s for s, _ in restarts], [sn for _, sn in restarts])
            for (s, sn), h in zip(restarts, hdr):
                assert h == w.start(s, sn)
        info, packets, nbytes = oc.pack_rows(rows, M, hole_rng)
        got, offsets, status = both(mux, info, packets, nbytes, flush, f"call {t}")
        seen_status |= set(status.tolist())
        pages += bytes(got).count(b"OggS")
        want, _ = w.call(rows, flush)                      # and the twin's own yardstick
        for s in range(n):
            assert bytes(got[offsets[s]:offsets[s + 1]]) == want[s], f"call {t}, stream {s} against the host writer"
    assert pages > n and seen_status == {0}
    mux.close()
    w.close()


def test_device_equals_host_twin_on_statuses(cuda):
    """small queue, small row cap, rows after e_o_s, rows of streams never started, packets above max_packet_bytes"""
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    n, M, R = 1100, 2000, 4
    rng = np.random.default_rng(5)
    mux = v.OggMux(setup, n, M, max_rows_per_stream=R, queue_bytes=3000)
    mux.start(list(range(0, n - 50)))                      # the last 50 are never started
    pno = [3] * n
    seen = set()
    for t in range(14):
        rows = []
        for s in range(n):
            k = int(rng.integers(0, 7))                    # 5, 6 rows: over the cap
            if rng.random() < 0.5:
                k = min(k, 1)
            for _ in range(k):
                size = int(rng.integers(0, M + 1)) if rng.random() < 0.98 else M + 1 + int(rng.integers(0, 40))
                rows.append((s, oc.payload(rng, size), 100 * pno[s], rng.random() < 0.02, pno[s]))
                pno[s] += 1
        order = rng.permutation(len(rows))
        info, packets, nbytes = oc.pack_rows([rows[i] for i in order], M + 64, rng)
        _, _, status = both(mux, info, packets, nbytes, t == 6, f"call {t}")
        seen |= set(status[:n].tolist())
    assert seen == {v.OggMux.OK, v.OggMux.EROWS, v.OggMux.EQUEUE, v.OggMux.ESTATE, v.OggMux.EPACKET}
    mux.close()


def test_out_capacity_below_the_bound_is_refused_on_the_host(cuda):
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    mux = v.OggMux(setup, 8, 4096)
    mux.start()
    info, packets, nbytes = oc.pack_rows([(3, b"abc", 5, True, 3)], 4096, holes=False)
    bound = int(v.lib.vbm_ogg_mux_out_bound(mux._h, 1))
    assert bound == mux.out_bound(1)
    out = torch.zeros(bound, dtype=torch.uint8, device=cuda)
    offsets = torch.full((9,), -7, dtype=torch.int64, device=cuda)
    status = torch.full((9,), -7, dtype=torch.int32, device=cuda)
    dp, dn = torch.from_numpy(packets).to(cuda), torch.from_numpy(nbytes).to(cuda)
    di = torch.from_numpy(info.view(np.uint8).copy()).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    args = (mux._h, dp.data_ptr(), 4096, dn.data_ptr(), di.data_ptr(), 1, 0, out.data_ptr())
    assert v.lib.vbm_ogg_mux_packets(*args, bound - 1, offsets.data_ptr(), status.data_ptr(), st) == -131
    torch.cuda.synchronize()
    assert (offsets == -7).all() and (status == -7).all() and not out.any()
    assert v.lib.vbm_ogg_mux_packets(*args, bound, offsets.data_ptr(), status.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert offsets.tolist() == [0, 0, 0, 0] + [27 + 1 + 3] * 5 and not status.any()
    assert bytes(out[:31].cpu().numpy())[:4] == b"OggS" and out[5] == 0x04
    # a host mux is refused by the device call and the other way round
    assert v.lib.vbm_ogg_mux_packets(mux._hh, *args[1:], bound, offsets.data_ptr(), status.data_ptr(), st) == -131
    mux.close()


# ---- end to end from PCM ---------------------------------------------------------------------------------------------

class Collector:
    """the rows and the muxed bytes of every call, kept on the device and copied out once"""

    def __init__(self, mux):
        self.mux, self.rows, self.outs = mux, [], []

    def take(self, info, packets, nbytes, flush=False):
        dev = self.mux.device
        if isinstance(info, torch.Tensor):
            dinfo = info.clone()
        else:
            dinfo = torch.from_numpy(np.ascontiguousarray(info).view(np.uint8).reshape(-1, 40).copy()).to(dev)
        out, offsets, status = self.mux.mux(info, packets, nbytes, flush)
        self.rows.append((dinfo, packets.clone(), nbytes.clone()))
        self.outs.append((out.clone(), offsets.clone(), status.clone()))

    def finish(self):
        """-> (per stream: muxed bytes over all calls, per stream: [(packetno, packet, granulepos, eos)] sorted)"""
        import vorbis_aotuv_lancer_amd as v
        n = self.mux.nstreams
        got = [[] for _ in range(n)]
        pk = [[] for _ in range(n)]
        torch.cuda.synchronize()
        for (out, offsets, status), (dinfo, packets, nbytes) in zip(self.outs, self.rows):
            out, offsets, status = out.cpu().numpy(), offsets.cpu().numpy(), status.cpu().numpy()
            assert not status.any(), np.flatnonzero(status)[:8]
            for s in range(n):
                got[s].append(bytes(out[offsets[s]:offsets[s + 1]]))
            rec = dinfo.cpu().numpy().reshape(-1, 40).view(np.dtype(v.PacketInfo))[:, 0]
            nb, data = nbytes.cpu().numpy(), packets.cpu().numpy()
            for k in np.flatnonzero(nb >= 0):
                r = rec[k]
                if r["stream"] >= 0:
                    pk[int(r["stream"])].append((int(r["packetno"]), bytes(data[k, :nb[k]]), int(r["granulepos"]), bool(r["eos"])))
        return [b"".join(g) for g in got], [sorted(p, key=lambda r: r[0]) for p in pk]


def check_streams(setup, mux, headers, got, pk, samples, comments, streams=None):
    import vorbis_aotuv_lancer_amd as v
    streams = range(mux.nstreams) if streams is None else streams
    files = []
    for s in streams:
        assert pk[s] and pk[s][-1][3] and [p[0] for p in pk[s]] == list(range(3, 3 + len(pk[s]))), f"stream {s}: packet numbers"
        want = v.write_ogg(setup, [p[1] for p in pk[s]], [(p[2], p[3]) for p in pk[s]], serialno=int(mux.serialnos[s]),
                           comments=comments)
        blob = headers[s] + got[s]
        assert blob == want, f"stream {s}: {len(blob)} bytes, write_ogg made {len(want)}"
        files.append(blob)
    for s, (pcm, rate) in zip(streams, v.decode_ogg(files)):
        assert pcm.shape[1] == samples[s], f"stream {s}: decoded {pcm.shape[1]} samples of {samples[s]}"


def drain_host_rounds(fe, col, multi):
    while True:
        if multi:
            info, packets, nbytes, counts = fe.encode_rounds(min_rounds=64, max_rounds=4)
        else:
            info, packets, nbytes = fe.encode_round()
        if len(info) == 0:
            break
        col.take(info.copy(), packets, nbytes)


@pytest.mark.parametrize("ch,rate,q,device_rounds", [(2, 44100, 0.5, True), (6, 48000, 0.8, True), (2, 44100, 0.5, False),
                                                     (6, 48000, 0.8, False)])
def test_pcm_to_ogg_end_to_end(cuda, monkeypatch, ch, rate, q, device_rounds):
    """64 streams; device-built rounds (no host read in the loop) or host-built compact rounds whose info records live
    on the host; three groups of streams end at different times, each after a complete drain through host-built
    rounds, whose rows go through the mux as well."""
    import vorbis_aotuv_lancer_amd as v
    monkeypatch.setenv("VBM_WORKSPACES", "4")
    NS, nwrites = 64, 14
    comments = ("TITLE=mux", "ARTIST=test")
    setup = v.Setup(ch, rate, q)
    lanes = v.lib.vbm_device_round_lanes(setup._h, NS)
    enc = v.Encoder(setup, NS, max_batch=max(lanes, NS))
    fe = v.FrontEnd(enc)
    mux = v.OggMux(setup, NS, enc.max_packet_bytes, serialnos=[0x7fff0000 + 3 * s for s in range(NS)], comments=comments)
    headers = mux.start()
    col = Collector(mux)
    extra = [0 if s % 3 == 0 else (2 if s % 3 == 1 else 5) for s in range(NS)]      # writes after the common part
    sig = [synth_signal(ch, rate, (nwrites + 5) * 1024, seed=300 + s, level=1.0 if s % 4 else 0.05) if s % 2 else
           burst_signal(ch, rate, (nwrites + 5) * 1024, seed=300 + s, period=9000) for s in range(NS)]
    allp = torch.from_numpy(np.stack(sig)).to(cuda)
    for c in range(nwrites):
        fe.write(allp[:, :, c * 1024:(c + 1) * 1024].contiguous())
        if device_rounds:
            info, packets, nbytes, counts = fe.encode_rounds_device(nrounds=2 if c % 4 else 3)
            col.take(info, packets, nbytes)
        else:
            info, packets, nbytes, counts = fe.encode_rounds(min_rounds=1, max_rounds=4)
            col.take(info.copy(), packets, nbytes)
    written = [nwrites] * NS
    for step in (0, 2, 5):
        live = [s for s in range(NS) if extra[s] > step]
        drain_host_rounds(fe, col, not device_rounds)
        ending = [s for s in range(NS) if extra[s] == step]
        fe.finish(ending)
        drain_host_rounds(fe, col, not device_rounds)
        nxt = {0: 2, 2: 5, 5: 5}[step]
        for c in range(step, nxt):
            if live:
                fe.write_streams(live, torch.stack([allp[s, :, written[s] * 1024:(written[s] + 1) * 1024] for s in live]).contiguous())
                for s in live:
                    written[s] += 1
                drain_host_rounds(fe, col, not device_rounds)
    col.take(np.zeros(0, oc.INFO), torch.zeros((0, enc.max_packet_bytes), dtype=torch.uint8, device=cuda),
             torch.zeros((0,), dtype=torch.int32, device=cuda), flush=True)
    got, pk = col.finish()
    assert len({len(p) for p in pk}) > 2
    check_streams(setup, mux, headers, got, pk, [w * 1024 for w in written], comments)
    mux.close()
    fe.close()
    enc.close()


def test_full_size_16384_streams(cuda, monkeypatch):
    """16384 stereo q5 streams, 24 writes through device-built rounds (the benchmarked path), every call muxed on the
    device; the rows of every call go to the host twin after the loop: equal bytes, offsets and status for every
    stream.  A sample of streams against write_ogg and the decoder."""
    import vorbis_aotuv_lancer_amd as v
    monkeypatch.setenv("VBM_WORKSPACES", "4")
    S, K, ch, rate, q, nwrites = 16384, 16, 2, 44100, 0.5, 24
    sigs = [burst_signal(ch, rate, nwrites * 1024, seed=400 + k, period=40000, level=1.0 if k % 5 else 0.05) for k in range(K)]
    base = torch.from_numpy(np.stack(sigs)).to(cuda)
    setup = v.Setup(ch, rate, q)
    lanes = v.lib.vbm_device_round_lanes(setup._h, S)
    enc = v.Encoder(setup, S, max_batch=lanes)
    fe = v.FrontEnd(enc)
    M = enc.max_packet_bytes
    mux = v.OggMux(setup, S, M)
    headers = mux.start()
    calls = []                                             # per call: device result and live rows, on the host

    def take(info, packets, nbytes, flush=False):
        out, offsets, status = mux.mux(info, packets, nbytes, flush)
        offs = offsets.cpu().numpy()                       # the one read a consumer makes per write
        nb = nbytes.cpu().numpy()
        live = np.flatnonzero(nb >= 0)
        rec = info.cpu().numpy().reshape(-1, 40).view(np.dtype(v.PacketInfo))[:, 0] if isinstance(info, torch.Tensor) \
            else np.ascontiguousarray(info).copy()
        width = int(nb[live].max()) if len(live) else 0
        data = packets[torch.from_numpy(live).to(cuda), :max(width, 1)].cpu().numpy() if len(live) else np.zeros((0, 1), np.uint8)
        calls.append((out[:int(offs[-1])].cpu().numpy(), offs, status.cpu().numpy(), rec[live].copy(), data, nb[live].copy(), flush))

    pattern = (2, 1, 1, 1)
    for c in range(nwrites):
        fe.write(base[:, :, c * 1024:(c + 1) * 1024].repeat(S // K, 1, 1).contiguous())
        info, packets, nbytes, counts = fe.encode_rounds_device(nrounds=3 if c < 6 else pattern[c % 4])
        take(info, packets, nbytes)
    assert fe.device_stats() and fe.refused_writes == 0
    torch.cuda.synchronize()
    for phase in range(2):
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                break
            take(info.copy(), packets, nbytes)
        if phase == 0:
            fe.finish()
    take(np.zeros(0, oc.INFO), torch.zeros((0, M), dtype=torch.uint8, device=cuda), torch.zeros((0,), dtype=torch.int32, device=cuda), True)

    # the host twin on the same rows
    total_bytes = 0
    row = np.zeros((1, M), np.uint8)
    for t, (out, offs, status, rec, data, nb, flush) in enumerate(calls):
        if len(row) < len(nb):
            row = np.zeros((len(nb), M), np.uint8)
        row[:len(nb), :data.shape[1]] = data
        hout, hoffs, hstatus = mux.mux_host(rec, row[:max(len(nb), 0)], nb, flush)
        assert not status.any() and np.array_equal(status, hstatus), f"call {t}: status"
        assert np.array_equal(offs, hoffs), f"call {t}: offsets"
        assert np.array_equal(out, hout), f"call {t}: bytes"
        total_bytes += len(out)
    assert total_bytes > S * nwrites * 300
    # a sample of streams against the host writer and the decoder
    sample = [0, 1, 5, 4097, 8191, 12345, 16383]
    pk = {s: [] for s in sample}
    got = {s: [] for s in sample}
    for out, offs, status, rec, data, nb, flush in calls:
        for s in sample:
            got[s].append(bytes(out[offs[s]:offs[s + 1]]))
            for k in np.flatnonzero(rec["stream"] == s):
                pk[s].append((int(rec["packetno"][k]), bytes(data[k, :nb[k]]), int(rec["granulepos"][k]), bool(rec["eos"][k])))
    gotl = [None] * S
    pkl = [None] * S
    for s in sample:
        gotl[s], pkl[s] = b"".join(got[s]), sorted(pk[s], key=lambda r: r[0])
    check_streams(setup, mux, headers, gotl, pkl, [nwrites * 1024] * S, (), streams=sample)
    mux.close()
    fe.close()
    enc.close()
