"""vbm_host_ogg_mux_packets (the paging rule of csrc/ogg_mux.h on the CPU) against the host writer vbm_ogg_stream_*,
byte for byte: several streams per call, streams without a row, rows shuffled across streams."""
import struct

import numpy as np
import pytest

import vorbis_aotuv_lancer_amd as v
from tests import oggmux_cases as oc

M_BIG = 70000


@pytest.fixture(scope="module")
def setup():
    return v.Setup(2, 44100, 0.5)


def host_runner(setup, n, M, **kw):
    mux = v.OggMux(setup, n, M, **kw)
    return mux, (lambda info, packets, nbytes, flush: mux.mux_host(info, packets, nbytes, flush)), \
        (lambda ids, serials: mux.start(ids, serials))


def pages_of(blob):
    """-> [(flags, granule, serialno, pageno, nseg, body bytes)]"""
    out, pos = [], 0
    while pos < len(blob):
        assert blob[pos:pos + 4] == b"OggS"
        _, flags, granule, sno, seq, _, nseg = struct.unpack_from("<BBqIIIB", blob, pos + 4)
        body = sum(blob[pos + 27:pos + 27 + nseg])
        out.append((flags, granule, sno, seq, nseg, body))
        pos += 27 + nseg + body
    return out


def test_directed_cases_match_the_host_writer(setup):
    rng = np.random.default_rng(11)
    scheds = oc.directed(rng, M_BIG, 16)
    case = oc.Case(scheds, M_BIG, seed=5, flush_at=(4, 9))
    mux, call, start = host_runner(setup, case.n, M_BIG)
    total = oc.run_case(case, call, start, setup)
    for s, blob in enumerate(total):      # a demuxer accepts what came out (CRC, page sequence, continuation flags)
        if "restart" not in scheds[s]:
            v.read_ogg(blob)
    mux.close()


def test_whole_streams_equal_write_ogg(setup):
    """no flush inside: header pages + muxed bytes == write_ogg of the stream's packets"""
    rng = np.random.default_rng(3)
    M, R = 9000, 16
    scheds = [oc.sched_sizes(M), oc.sched_ones(R), oc.sched_253_600(R), oc.sched_big(M), oc.sched_random(rng, M, R)]
    case = oc.Case(scheds, M, seed=8, flush_at=())
    mux, call, start = host_runner(setup, case.n, M)
    total = oc.run_case(case, call, start, setup)
    packets = [[] for _ in scheds]
    for _, rows, _, _ in case.steps():
        for s, data, gp, eos, pno in rows:
            packets[s].append((pno, data, gp, eos))
    for s in range(case.n):
        pk = sorted(packets[s], key=lambda r: r[0])
        assert total[s] == v.write_ogg(setup, [p[1] for p in pk], [(p[2], p[3]) for p in pk], serialno=s)
    mux.close()


def test_253_one_byte_packets_then_600(setup):
    """the case random sizes do not reach: a page forced at 255 segments inside a packet, then a continued page"""
    n = 3
    mux = v.OggMux(setup, n, 4096)
    hdr = mux.start()
    rng = np.random.default_rng(1)
    rows, gp = [], 0
    sizes = [1] * 253 + [600, 10, 10, 10]
    for k, size in enumerate(sizes):
        gp += 128
        rows.append((1, oc.payload(rng, size), gp, k == len(sizes) - 1, 3 + k))
    got = b""
    for at in range(0, len(rows), 16):
        info, packets, nbytes = oc.pack_rows(rows[at:at + 16][::-1], 4096)
        out, offsets, status = mux.mux_host(info, packets, nbytes)
        assert not status.any() and offsets[1] == 0 and offsets[2] == offsets[3]
        got += bytes(out)
    want = v.write_ogg(setup, [r[1] for r in rows], [(r[2], r[3]) for r in rows], serialno=1)
    assert hdr[1] + got == want
    pg = pages_of(got)
    assert len(pg) == 2
    assert pg[0][4] == 255 and pg[0][5] == 763 and not pg[0][0] & 0x04 and pg[0][1] == 128 * 253
    assert pg[1][4] == 4 and pg[1][5] == 120 and pg[1][0] == 0x05
    mux.close()


@pytest.mark.parametrize("seed", range(8))
def test_random_sequences(setup, seed):
    """8 x 40 = 320 seeded random schedules"""
    rng = np.random.default_rng(100 + seed)
    M, R = 6000, 8
    scheds = [oc.sched_random(rng, M, R, steps=int(rng.integers(4, 24))) for _ in range(40)]
    case = oc.Case(scheds, M, seed=seed, flush_at=(int(rng.integers(0, 12)),), delays=[int(rng.integers(0, 5)) for _ in scheds])
    mux, call, start = host_runner(setup, case.n, M, max_rows_per_stream=R)
    oc.run_case(case, call, start, setup)
    mux.close()


def test_row_after_eos_is_refused_and_others_go_on(setup):
    mux = v.OggMux(setup, 3, 4096)
    mux.start()
    w = oc.Writer(setup, 3)
    for s in range(3):
        w.start(s, s)
    rng = np.random.default_rng(2)
    rows = [(0, oc.payload(rng, 100), 10, True, 3), (1, oc.payload(rng, 200), 10, False, 3), (2, oc.payload(rng, 5000 - 904), 10, False, 3)]
    out, offsets, status = mux.mux_host(*oc.pack_rows(rows, 4096))
    want, _ = w.call(rows, False)
    assert [bytes(out[offsets[s]:offsets[s + 1]]) for s in range(3)] == want and not status.any()
    # the host writer refuses a packet after e_o_s ...
    with pytest.raises(v.VbmError):
        w.os[0].packetin(b"abc", 20)
    # ... and so does the mux, for that stream only
    rows = [(0, b"abc", 20, False, 4), (1, oc.payload(rng, 4096), 20, False, 4), (2, oc.payload(rng, 4096), 20, True, 4)]
    out, offsets, status = mux.mux_host(*oc.pack_rows(rows, 4096))
    want, _ = w.call(rows[1:], False)
    assert list(status) == [v.OggMux.ESTATE, 0, 0, 0]
    assert [bytes(out[offsets[s]:offsets[s + 1]]) for s in range(3)] == want and offsets[1] == 0
    # a slot that was never started refuses rows as well
    fresh = v.OggMux(setup, 2, 4096)
    out, offsets, status = fresh.mux_host(*oc.pack_rows([(1, b"x", 1, False, 3)], 4096))
    assert list(status) == [0, v.OggMux.ESTATE, 0] and offsets[-1] == 0
    # rows that name no stream of the mux are counted
    out, offsets, status = fresh.mux_host(*oc.pack_rows([(2, b"x", 1, False, 3), (5, b"y", 1, False, 3)], 4096))
    assert status[2] == 2
    fresh.close()
    mux.close()
    w.close()


def test_rows_per_stream_cap(setup):
    mux = v.OggMux(setup, 2, 4096, max_rows_per_stream=4)
    mux.start()
    rows = [(0, b"a" * 9, 10 + k, False, 3 + k) for k in range(5)] + [(1, b"b" * 9, 10 + k, False, 3 + k) for k in range(4)]
    out, offsets, status = mux.mux_host(*oc.pack_rows(rows, 4096), flush=True)
    assert list(status) == [v.OggMux.EROWS, 0, 0]
    assert offsets[1] == 0 and offsets[2] == 27 + 4 + 36
    # stays refused until the slot starts again
    out, offsets, status = mux.mux_host(*oc.pack_rows([(0, b"c", 30, False, 8)], 4096), flush=True)
    assert status[0] == v.OggMux.EROWS and offsets[-1] == 0
    mux.start([0], [77])
    out, offsets, status = mux.mux_host(*oc.pack_rows([(0, b"c", 30, False, 3)], 4096), flush=True)
    assert status[0] == 0 and offsets[1] == 27 + 1 + 1
    mux.close()


def test_queue_capacity_status(setup):
    """a queue smaller than the rule can leave: the packet that would not fit is refused with a status, nothing is
    written out of bounds and nothing is dropped silently"""
    mux = v.OggMux(setup, 2, 4096, queue_bytes=1000)
    mux.start()
    w = oc.Writer(setup, 2)
    w.start(0, 0), w.start(1, 1)
    rng = np.random.default_rng(4)
    first = [(0, oc.payload(rng, 600), 10, False, 3), (1, oc.payload(rng, 600), 10, False, 3)]
    out, offsets, status = mux.mux_host(*oc.pack_rows(first, 4096))
    assert not status.any() and offsets[-1] == 0
    second = [(0, oc.payload(rng, 401), 20, False, 4), (1, oc.payload(rng, 400), 20, False, 4)]
    out, offsets, status = mux.mux_host(*oc.pack_rows(second, 4096))
    assert list(status) == [v.OggMux.EQUEUE, 0, 0] and offsets[-1] == 0
    # stream 0 kept what it had: a flush brings out exactly its first packet; stream 1 both
    out, offsets, status = mux.mux_host(*oc.pack_rows([], 4096), flush=True)
    w.call(first, False)
    w.call(second[1:], False)
    want, _ = w.call([], True)
    assert [bytes(out[offsets[s]:offsets[s + 1]]) for s in range(2)] == want
    assert status[0] == v.OggMux.EQUEUE
    mux.close()
    w.close()


def test_packet_above_max_packet_bytes(setup):
    mux = v.OggMux(setup, 1, 300)
    mux.start()
    out, offsets, status = mux.mux_host(*oc.pack_rows([(0, b"z" * 301, 5, False, 3)], 512), flush=True)
    assert status[0] == v.OggMux.EPACKET and offsets[-1] == 0
    mux.close()


def test_out_capacity_below_the_bound_is_einval_and_changes_nothing(setup):
    mux = v.OggMux(setup, 2, 4096)
    mux.start()
    rng = np.random.default_rng(6)
    rows = [(0, oc.payload(rng, 100), 10, False, 3), (1, oc.payload(rng, 50), 10, True, 3)]
    info, packets, nbytes = oc.pack_rows(rows, 4096, holes=False)
    bound = mux.out_bound(2)
    out = np.zeros(bound, np.uint8)
    offsets, status = np.full(3, -7, np.int64), np.full(3, -7, np.int32)
    args = (mux._hh, packets.ctypes.data, 4096, nbytes.ctypes.data, info.ctypes.data, 2, 0, out.ctypes.data)
    rc = v.lib.vbm_host_ogg_mux_packets(*args, bound - 1, offsets.ctypes.data, status.ctypes.data)
    assert rc == -131 and b"vbm_ogg_mux_out_bound" in v.lib.vbm_last_error()
    assert (offsets == -7).all() and (status == -7).all() and not out.any()
    # bad arguments are refused the same way
    assert v.lib.vbm_host_ogg_mux_packets(mux._hh, None, 4096, nbytes.ctypes.data, info.ctypes.data, 2, 0, out.ctypes.data,
                                          bound, offsets.ctypes.data, status.ctypes.data) == -131
    assert v.lib.vbm_host_ogg_mux_packets(mux._hh, packets.ctypes.data, 100, nbytes.ctypes.data, info.ctypes.data, 2, 0,
                                          out.ctypes.data, bound, offsets.ctypes.data, status.ctypes.data) == -131
    # the state is as it was: the same call with enough room gives what the writer gives
    assert v.lib.vbm_host_ogg_mux_packets(*args, bound, offsets.ctypes.data, status.ctypes.data) == 0
    w = oc.Writer(setup, 2)
    w.start(0, 0), w.start(1, 1)
    want, _ = w.call(rows, False)
    assert [bytes(out[offsets[s]:offsets[s + 1]]) for s in range(2)] == want and not status.any()
    mux.close()
    w.close()


@pytest.mark.parametrize("M", [300, 1500, 4096])
def test_adversarial_schedule_stays_within_the_bound(setup, M):
    """every stream holds the largest queue on which no page is due, then gets max_rows_per_stream largest packets with
    e_o_s on the last: the call's output is within vbm_ogg_mux_out_bound and equals the host writer's"""
    n, R = 4, 16
    mux = v.OggMux(setup, n, M, max_rows_per_stream=R)
    mux.start()
    w = oc.Writer(setup, n)
    for s in range(n):
        w.start(s, s)
    rng = np.random.default_rng(M)
    # the largest queue without a page due: four largest packets (4M), or packets up to 4096 bytes and one largest more
    fill = [[M] * 4, [M] * (4096 // M) + [4096 % M] * (1 if 4096 % M else 0) + [M], [0] * 254, [M] * 3 + [M - 1]]
    pno = [3] * n
    calls = max(len(f) for f in fill)
    for k in range(0, calls, R):
        rows = []
        for s in range(n):
            for size in fill[s][k:k + R]:
                rows.append((s, oc.payload(rng, size), pno[s], False, pno[s]))
                pno[s] += 1
        out, offsets, status = mux.mux_host(*oc.pack_rows(rows, M, rng))
        want, _ = w.call(rows, False)
        assert offsets[-1] == 0 and not any(want) and not status.any()      # no page is due on these queues
    queued = [sum(f) for f in fill]
    rows = []
    for s in range(n):
        for k in range(R):
            rows.append((s, oc.payload(rng, M), pno[s], k == R - 1, pno[s]))
            pno[s] += 1
    info, packets, nbytes = oc.pack_rows(rows, M, holes=False)
    out, offsets, status = mux.mux_host(info, packets, nbytes)
    want, _ = w.call(rows, False)
    assert [bytes(out[offsets[s]:offsets[s + 1]]) for s in range(n)] == want and not status.any()
    assert offsets[-1] > sum(queued) + n * R * M      # everything queued went out in this one call
    assert offsets[-1] <= mux.out_bound(len(rows))
    mux.close()
    w.close()


def test_mid_stream_flush(setup):
    mux = v.OggMux(setup, 2, 4096)
    hdr = mux.start()
    rng = np.random.default_rng(9)
    rows = [(0, oc.payload(rng, 300), 100, False, 3), (1, oc.payload(rng, 20), 100, False, 3)]
    out, offsets, status = mux.mux_host(*oc.pack_rows(rows, 4096), flush=True)
    pg = pages_of(bytes(out[:offsets[1]]))
    assert len(pg) == 1 and pg[0][3] == pages_of(hdr[0])[-1][3] + 1 and pg[0][5] == 300 and pg[0][1] == 100
    out, offsets, status = mux.mux_host(*oc.pack_rows([], 4096), flush=True)      # nothing queued: nothing comes out
    assert offsets[-1] == 0
    mux.close()
