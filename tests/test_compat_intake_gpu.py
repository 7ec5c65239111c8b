"""PCM intake of the drop-in shim (include/vorbis_compat.h): writes that do not go through the pinned arena — larger than
a stream's arena region, a second and third write before the pool's next round, more written than half of what was
asked for, no arena at all — streams of different write sizes in one upload, the end declared with writes still
queued, and the largest write a stream takes.  Every stream equals the oracle given the same writes, drains and end."""
import ctypes as C

import pytest

from tests import compat, orc
from tests import intake_cases as ic

pytestmark = pytest.mark.gpu
STEREO_Q5 = (2, 44100, 0.5)
FINISH = "finish"


@pytest.fixture()
def dll():
    import vorbis_aotuv_lancer_amd as v
    d = compat.bind(C.CDLL(v.COMPAT_LIB_PATH))

    def knobs(carve=1, defer=0, pool=None):
        """(the pool size has no "unset": like tests/test_compat_gpu.py, every test that depends on it sets it)"""
        for request, value in ((2, carve), (5, defer), (1, pool)):
            if value is not None:
                d.vorbis_mi355x_ctl(request, C.byref(C.c_int(value)))
    d.knobs = knobs
    knobs()
    yield d
    knobs()


def run_pool(dll, oracle, cls, signals, turns):
    """turns[s]: one list per application turn — write sizes (("as", buffer_vals, n): vorbis_analysis_buffer of another
    size than is written; ("refused", n): a write that must return OV_EINVAL and bring nothing), FINISH last.  A turn:
    every stream makes its calls, then every stream is drained (examples/encoder_example.c:190-235 per stream).
    Returns (got, want) per stream."""
    n = len(signals)
    ss = [compat.Stream(dll, *cls) for _ in range(n)]
    got, at, schedule = [[] for _ in range(n)], [0] * n, []
    try:
        for k in range(max(len(t) for t in turns)):
            for s in range(n):
                for item in (turns[s][k] if k < len(turns[s]) else []):
                    if item == FINISH:
                        assert ss[s].finish() == 0
                        schedule.append(("finish", [s]))
                        continue
                    if isinstance(item, tuple):                       # ("as", buffer_vals, n) or ("refused", n)
                        kind, buf, vals = item[0], item[1], item[-1]
                    else:
                        kind, buf, vals = "write", item, item
                    pcm = signals[s][:, at[s]:at[s] + vals]
                    assert pcm.shape[1] == vals, (s, at[s], vals)
                    if kind == "refused":
                        assert ss[s].write(pcm) == compat.OV_EINVAL
                        continue
                    rc = ss[s].write(pcm) if kind == "write" else ss[s].write_as(pcm, buf)
                    assert rc == 0, (s, k, item, rc)
                    at[s] += vals
                    schedule.append(("write", {s: vals}))
            for s in range(n):
                if k < len(turns[s]):
                    got[s].extend(ss[s].drain())
            schedule.append(("drain",))
        for s in range(n):
            assert ss[s].blockout() == 0                              # stream over: nothing more (lib/block.c:566)
    finally:
        for st in ss:
            st.close()
    want = ic.oracle_run(oracle, orc.Setup(oracle, *cls), signals, schedule)
    return got, [[(m[:3] + m[4:], p) for m, p in want[s][0]] for s in range(n)]


def compare(got, want):
    for s in range(len(want)):
        assert [m for m, _ in got[s]] == [m for m, _ in want[s]], f"stream {s}: block sequence differs from the oracle"
        bad = [i for i in range(len(want[s])) if got[s][i][1] != want[s][i][1]]
        assert not bad, f"stream {s}: packet {bad[0]} of {len(want[s])} differs from the oracle"
        assert got[s][-1][0][3] == 1                                  # e_o_s on the last packet


def turns_of(sizes):
    return [[n] for n in sizes] + [[FINISH]]


def signals_for(cls, lengths, seed=930):
    return [ic.burst_signal(cls[0], cls[1], L, seed=seed + s, level=1.0 if s % 3 else 0.2) for s, L in enumerate(lengths)]


POOL_SIZES = [333, 1024, 1025, 2048, 4097, 333, 1024, 1025, 2048, 4097]


def pool_case(total=24000):
    lengths = [total + 500 * s for s in range(len(POOL_SIZES))]       # the streams end at different times
    return lengths, [turns_of(ic.size_list(str(n), 2048, L)) for n, L in zip(POOL_SIZES, lengths)]


@pytest.mark.parametrize("defer", [0, 1])
def test_write_sizes_in_one_pool(oracle, cuda, dll, defer):
    """ten streams of one pool, each with its own write size: up to 1024 samples through the arena, the rest copied,
    every upload holding groups of different length (VORBIS_MI355X_DEFER_BLOCKS: same packets, later delivery)"""
    dll.knobs(defer=defer, pool=10)
    lengths, turns = pool_case()
    compare(*run_pool(dll, oracle, STEREO_Q5, signals_for(STEREO_Q5, lengths), turns))


@pytest.mark.parametrize("arena_vals", [0, 4096])
def test_arena_size(oracle, cuda, dll, monkeypatch, arena_vals):
    """VORBIS_MI355X_ARENA_VALS (read when a pool is made): no arena, every write copied; 4096 samples per region,
    only the 4097-sample writes copied"""
    monkeypatch.setenv("VORBIS_MI355X_ARENA_VALS", str(arena_vals))
    dll.knobs(pool=10)
    # the setting took effect (a pool left over from an earlier test would still have the default arena): a request
    # the arena serves reports a region's size as vd->pcm_storage, one it cannot serve the host buffer's (twice the request)
    probe = compat.Stream(dll, *STEREO_Q5)
    assert dll.vorbis_analysis_buffer(probe.vd, 1000)
    storage = int(probe.vd.pcm_storage)
    probe.close()
    assert storage == (arena_vals or 2000), storage
    times = (C.c_double * 8)()
    dll.vorbis_mi355x_ctl(6, times)
    staged = times[1]
    lengths, turns = pool_case(total=16000)
    compare(*run_pool(dll, oracle, STEREO_Q5, signals_for(STEREO_Q5, lengths, seed=950), turns))
    dll.vorbis_mi355x_ctl(6, times)
    assert times[1] > staged                                         # writes went up through staging copies


def test_several_writes_between_blockouts(oracle, cuda, dll):
    """two and three writes per turn: the first stays in the stream's arena region, which the later ones find pending
    and are copied; vorbis_analysis_buffer(1024) followed by vorbis_analysis_wrote(700); seven 4097-sample writes in a
    turn, more than the device buffer holds (the upload carves blocks until the next write fits)"""
    dll.knobs(pool=10)
    per_turn = [[1024, 1024], [1024, 700, 333], [("as", 1024, 700)], [4097] * 7, [("as", 1024, 700), 1024]]
    turns, lengths = [], []
    for pattern in per_turn:
        n = sum(x[2] if isinstance(x, tuple) else x for x in pattern)
        nturns = max(2, 26000 // n + 1)
        turns.append([list(pattern) for _ in range(nturns)] + [[FINISH]])
        lengths.append(nturns * n)
    compare(*run_pool(dll, oracle, STEREO_Q5, signals_for(STEREO_Q5, lengths, seed=960), turns))


def test_end_of_stream_with_writes_still_queued(oracle, cuda, dll):
    """the end is declared in the same turn as the last writes, before any vorbis_analysis_blockout has made them go
    up: stream 1 never asked for a block at all (test/write_read.c:95-99 of the reference does the same)"""
    dll.knobs(pool=10)
    turns = [turns_of([1024] * 9)[:-1] + [[1024, 333, FINISH]],
             [[1024, 1024, 700, FINISH]],
             [[2049, 2049], [2049, 100, FINISH]]]
    lengths = [9 * 1024 + 1357, 2748, 2 * 2049 + 2149]
    compare(*run_pool(dll, oracle, STEREO_Q5, signals_for(STEREO_Q5, lengths, seed=970), turns))


@pytest.mark.parametrize("cls", [STEREO_Q5, (1, 8000, 0.5)], ids=["2ch-44100", "1ch-8000"])
def test_write_larger_than_the_buffer_takes(oracle, cuda, dll, cls):
    """A write of more than the front end's capacity (13 long blocks) could never go up: it is refused by
    vorbis_analysis_wrote itself with OV_EINVAL, as is every write that might find the buffer too full even when
    drained, and nothing is queued: the stream takes ordinary writes afterwards and equals the
    oracle given the accepted writes only, a second stream of the pool never notices, and a third takes a first write
    of exactly the limit."""
    dll.knobs(pool=10)
    bs1 = ic.blocksizes(orc.Setup(oracle, *cls))[1]
    capacity = ic.CAPACITY_BLOCKS * bs1
    limit = capacity - (3 * bs1 // 2 + 448)
    ordinary = [[1024]] * 12
    turns = [[[("refused", capacity + 1)]] + ordinary[:5] + [[("refused", limit + 1), 1024]] + ordinary[:4] + [[FINISH]],
             ordinary + [[FINISH]],
             [[limit]] + ordinary[:3] + [[limit]] + [[FINISH]]]
    lengths = [capacity + 8 * 1024, 12 * 1024, 2 * limit + 3 * 1024]
    compare(*run_pool(dll, oracle, cls, signals_for(cls, lengths, seed=980), turns))
