"""The encoder tests' own toolkit (tests/encode_oracle.py) on the CPU oracle and on made-up arrays: the walk's options,
the record, the lock-step schedule, and every comparer against doctored data — each must pass on the oracle's own data
and raise AssertionError on a wrong byte, bit, flag or record.

One small corpus: stereo 44100 q0.5, burst_signal(2, 44100, 44100, seed=3) (94 blocks, all four block types), a mono
8000 class (one block size) and one managed setup."""
import numpy as np
import pytest

from tests import encode_oracle as eo
from tests.signals import burst_signal

STEREO = (2, 44100, 0.5)
STAGES_F = ("mdct_raw", "logfft", "logmdct", "noise", "tone", "logmask", "mdct", "epeak", "npeak", "poste")
STAGES_I = ("post_valid", "nonzero", "residue")


def stereo_pcm():
    return burst_signal(2, 44100, 44100, seed=3)


@pytest.fixture(scope="module")
def full(oracle):
    return eo.walk(oracle, *STEREO, pcm=stereo_pcm(), key="toolkit")


@pytest.fixture(scope="module")
def mono(oracle):
    return eo.walk(oracle, 1, 8000, 0.5, pcm=burst_signal(1, 8000, 16384, seed=4), key="toolkit mono")


@pytest.fixture(scope="module")
def managed(oracle):
    return eo.walk(oracle, 2, 44100, bitrate=128000, pcm=stereo_pcm()[:, :20480], key="toolkit managed")


def same_blocks(a, b, fields):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in fields:
            assert np.array_equal(np.asarray(x[f]), np.asarray(y[f])), f


# ---- walk ---------------------------------------------------------------------------------------------------------------
def test_walk_corpus(full, mono):
    assert len(full) == 94 and {b["block_mode"] for b in full} == {0, 1, 2, 3}
    assert {b["block_mode"] for b in mono} == {0, 1} and len({b["N"] for b in mono}) == 1


def test_walk_unfinished_is_a_strict_prefix(oracle, full):
    open_ = eo.walk(oracle, *STEREO, pcm=stereo_pcm(), finish=False)
    assert len(open_) == 86 < len(full)
    assert eo.records(open_) == eo.records(full)[:len(open_)]
    same_blocks(open_, full[:len(open_)], STAGES_F + STAGES_I + ("pcm",))
    assert [b["eos"] for b in full] == [0] * (len(full) - 1) + [1] and not any(b["eos"] for b in open_)


def test_walk_without_capture_gives_the_same_records(oracle, full):
    assert eo.records(eo.walk(oracle, *STEREO, pcm=stereo_pcm(), capture=False)) == eo.records(full)


def test_walk_keep(oracle, full):
    keep = ("lW", "nW", "block_mode", "pcm", "packet", "tone", "blobs")       # (a VBR block has no blobs)
    kept = eo.walk(oracle, *STEREO, pcm=stereo_pcm(), keep=keep)
    assert all(set(b) == set(keep) - {"blobs"} for b in kept)
    same_blocks(kept, full, set(keep) - {"blobs"})


def test_walk_cache(oracle, full):
    assert eo.walk(oracle, *STEREO, pcm=stereo_pcm(), key="toolkit") is full
    assert eo.walk(oracle, *STEREO, pcm=stereo_pcm(), key="toolkit", finish=False) is not full
    assert eo.walk(oracle, *STEREO, pcm=stereo_pcm()) is not full
    made = []
    lazy = [eo.walk(oracle, *STEREO, pcm=lambda: made.append(1) or stereo_pcm()[:, :8192], key="toolkit lazy") for _ in range(2)]
    assert lazy[0] is lazy[1] and len(made) == 1               # a maker is called only when the result is not cached
    assert eo.records(lazy[0]) == eo.records(eo.walk(oracle, *STEREO, pcm=stereo_pcm()[:, :8192]))
    with pytest.raises(ValueError):
        full[0]["pcm"][0, 0] = 1.0
    with pytest.raises(ValueError):
        full[-1]["residue"][0, 0] = 1


def test_walk_in_one_write(oracle):
    pcm = stereo_pcm()[:, :5000]
    one = eo.walk(oracle, *STEREO, pcm=pcm, chunk=None)
    assert eo.records(one) == eo.records(eo.walk(oracle, *STEREO, pcm=pcm, chunk=5000))
    assert eo.records(one) != eo.records(eo.walk(oracle, *STEREO, pcm=pcm, chunk=64))       # the delivery matters


def test_walk_on_block(oracle, managed):
    seen = []
    blks = eo.walk(oracle, 2, 44100, bitrate=128000, pcm=stereo_pcm()[:, :20480], on_block=lambda st, b, ended: seen.append((b["sequence"], ended)))
    assert [s for s, _ in seen] == [b["sequence"] for b in blks] == [b["sequence"] for b in managed]
    tail = [ended for _, ended in seen]
    assert tail == sorted(tail) and tail[0] is False and tail[-1] is True


# ---- record -------------------------------------------------------------------------------------------------------------
def test_record_from_a_block_and_from_a_packet_info_row(full):
    rows = np.zeros(len(full), np.dtype([("stream", np.int32)] + [(f, np.int64 if f in ("granulepos", "packetno") else np.int32)
                                                                    for f in eo.RECORD_FIELDS]))
    for row, b in zip(rows, full):
        for f in eo.RECORD_FIELDS:
            row[f] = b["sequence" if f == "packetno" else f]
    assert [eo.record(row, b["packet"]) for row, b in zip(rows, full)] == eo.records(full)
    meta, packet = eo.record(full[5])
    assert meta == tuple(full[5][f] for f in ("lW", "W", "nW", "block_mode", "eos", "granulepos", "sequence"))
    assert packet == full[5]["packet"] and all(type(x) is int for x in meta)


# ---- lockstep -----------------------------------------------------------------------------------------------------------
def test_lockstep(full):
    streams = [full, full[:40], full[10:75]]
    calls = list(eo.lockstep(streams))
    seen = sorted((int(m), k) for k, mode, present, ids, blks in calls for m in present)
    assert seen == sorted((m, k) for m, s in enumerate(streams) for k in range(len(s)))          # every block once
    for k, mode, present, ids, blks in calls:
        assert list(ids) == present == sorted(present) and [b["block_mode"] for b in blks] == [mode] * len(present)
        assert all(blks[i] is streams[m][k] for i, m in enumerate(present))
    order = [(k, mode) for k, mode, *_ in calls]
    assert order == sorted(order) and len(set(order)) == len(order)                              # ascending type within a k
    assert max(len({mode for k2, mode, *_ in calls if k2 == k}) for k in range(40)) > 1           # (some k has two types)


def test_lockstep_replicas(full):
    streams = [full, full[:40], full[10:75]]
    K, R = 3, 3
    plain = list(eo.lockstep(streams))
    for (k, mode, present, ids, blks), one in zip(eo.lockstep(streams, R=R), plain):
        assert (k, mode, present) == one[:3] and blks == one[4]
        assert ids.dtype == np.int32 and len(ids) == R * len(present)
        assert list(ids) == [r * K + m for r in range(R) for m in present]
        for row, s in enumerate(ids):
            assert s % K == present[row % len(present)]                                          # the row-to-signal rule


def test_lockstep_shortest(full):
    streams = [full, full[:40], full[10:75]]
    short = list(eo.lockstep(streams, stop="shortest"))
    assert {k for k, *_ in short} == set(range(40))
    assert sorted(m for k, _, present, _, _ in short for m in present if k == 39) == [0, 1, 2]
    assert [c[:3] for c in short] == [c[:3] for c in eo.lockstep(streams) if c[0] < 40]


# ---- comparers ----------------------------------------------------------------------------------------------------------
def rows_of(blks, width=None):
    """what a call would fetch for these blocks: stage -> array, and the packet buffer with its lengths"""
    got = {name: np.concatenate([np.atleast_1d(b[name]) for b in blks]).copy() for name in STAGES_F + STAGES_I}
    width = width or max(len(b["packet"]) for b in blks) + 8
    packets = np.zeros((len(blks), width), np.uint8)
    for i, b in enumerate(blks):
        packets[i, :len(b["packet"])] = np.frombuffer(b["packet"], np.uint8)
    return got, packets, np.array([len(b["packet"]) for b in blks], np.int32)


def long_blocks(full):
    blks = [b for b in full if b["block_mode"] == 3 and b["nonzero"].all()][:3]
    assert len(blks) == 3
    return blks


def test_compare_packets(full):
    blks = long_blocks(full)
    want = [b["packet"] for b in blks]
    _, packets, nbytes = rows_of(blks)
    eo.compare_packets(packets, nbytes, want, "ok", zero_tail=True)
    short = nbytes.copy()
    short[1] -= 1
    with pytest.raises(AssertionError, match="packet length"):
        eo.compare_packets(packets, short, want, "one byte short")
    flipped = packets.copy()
    flipped[2, 17] ^= 0x10
    with pytest.raises(AssertionError, match="first differing byte.*17"):
        eo.compare_packets(flipped, nbytes, want, "flipped byte")
    tail = packets.copy()
    tail[0, nbytes[0] + 3] = 1
    eo.compare_packets(tail, nbytes, want, "tail ignored")
    with pytest.raises(AssertionError, match="not zero past the packet"):
        eo.compare_packets(tail, nbytes, want, "tail", zero_tail=True)
    with pytest.raises(AssertionError):
        eo.compare_packets(packets[:2], nbytes[:2], want, "a row missing")


def test_compare_block_call(full):
    blks = long_blocks(full)
    got, _, _ = rows_of(blks)
    eo.compare_block_call(got, blks, 2, STAGES_F, STAGES_I, label="ok")

    def doctored(name, change):
        bad = dict(got)
        bad[name] = got[name].copy()
        change(bad[name])
        return bad

    def flip_bit(x):
        x.view(np.uint32)[1, 100] ^= 1

    with pytest.raises(AssertionError, match="logmask"):
        eo.compare_block_call(doctored("logmask", flip_bit), blks, 2, STAGES_F, STAGES_I)
    eo.compare_block_call(doctored("logmask", flip_bit), blks, 2, [s for s in STAGES_F if s != "logmask"], STAGES_I)

    # -0.0 against 0.0: equal as floats, not as bits
    zeros = [dict(b, mdct=np.zeros_like(b["mdct"])) for b in blks]
    z = dict(got, mdct=np.zeros_like(got["mdct"]))
    eo.compare_block_call(z, zeros, 2, ("mdct",), ())
    z["mdct"][3, 7] = -0.0
    assert z["mdct"][3, 7] == 0.0
    with pytest.raises(AssertionError, match="mdct"):
        eo.compare_block_call(z, zeros, 2, ("mdct",), ())

    def clear_flag(x):
        x[2] ^= 1

    with pytest.raises(AssertionError, match="nonzero"):
        eo.compare_block_call(doctored("nonzero", clear_flag), blks, 2, STAGES_F, STAGES_I)

    def residue_of_channel_1(x):
        x[3, 5] += 1        # row 3 = block 1, channel 1

    with pytest.raises(AssertionError, match="residue"):
        eo.compare_block_call(doctored("residue", residue_of_channel_1), blks, 2, STAGES_F, STAGES_I)
    with pytest.raises(AssertionError, match="residue"):
        eo.compare_block_call(doctored("residue", residue_of_channel_1), blks, 2, STAGES_F, STAGES_I, res1_channels=(0,))
    eo.compare_block_call(doctored("residue", residue_of_channel_1), blks, 2, STAGES_F, STAGES_I, res1_channels=(1,))
    with pytest.raises(AssertionError, match="shape"):
        eo.compare_block_call(doctored("npeak", lambda x: None) | {"npeak": got["npeak"][:-1]}, blks, 2, STAGES_F, STAGES_I)


def test_compare_block_call_one_block_size(mono):
    blks = [b for b in mono if b["block_mode"] == 1][:2]
    got, packets, nbytes = rows_of(blks)
    eo.compare_block_call(got, blks, 1, STAGES_F, STAGES_I)
    eo.compare_packets(packets, nbytes, [b["packet"] for b in blks], "mono", zero_tail=True)
    got["tone"] = got["tone"].copy()
    got["tone"].view(np.uint32)[0, 0] ^= 0x80000000
    with pytest.raises(AssertionError, match="tone"):
        eo.compare_block_call(got, blks, 1, STAGES_F, STAGES_I)


def test_compare_records(full):
    want = eo.records(full)
    eo.compare_records(list(want), want, "ok")
    swapped = list(want)
    swapped[10], swapped[11] = swapped[11], swapped[10]
    with pytest.raises(AssertionError, match="block sequence differs.*record 10"):
        eo.compare_records(swapped, want, "reordered")
    with pytest.raises(AssertionError, match="block sequence differs.*record 93"):
        eo.compare_records(want[:-1], want, "last record missing")
    with pytest.raises(AssertionError, match="block sequence differs"):
        eo.compare_records(want + want[-1:], want, "one record too many")
    wrong = list(want)
    wrong[20] = (wrong[20][0], wrong[20][1][:-1] + bytes([wrong[20][1][-1] ^ 1]))
    with pytest.raises(AssertionError, match="packet 20"):
        eo.compare_records(wrong, want, "a flipped bit")
    field = list(want)
    field[30] = (field[30][0][:5] + (field[30][0][5] + 1,) + field[30][0][6:], field[30][1])
    with pytest.raises(AssertionError, match="record 30"):
        eo.compare_records(field, want, "granulepos")


def test_compare_blobs(managed):
    blks = [b for b in managed if b["block_mode"] == 3][:2]
    width = max(max(b["blob_bytes"]) for b in blks) + 4

    def blobs():
        out = []
        for kb in range(15):
            bp = np.zeros((len(blks), width), np.uint8)
            for i, b in enumerate(blks):
                bp[i, :len(b["blobs"][kb])] = np.frombuffer(b["blobs"][kb], np.uint8)
            out.append((bp, np.array([b["blob_bytes"][kb] for b in blks], np.int32)))
        return out

    choice = np.array([b["choice"] for b in blks])
    assert eo.compare_blobs(blobs(), choice, blks, "ok") == 0
    bad = blobs()
    bad[9][0][1, 11] ^= 4
    with pytest.raises(AssertionError, match="blob bytes"):
        eo.compare_blobs(bad, choice, blks, "flipped")
    bad = blobs()
    bad[0][1][0] += 1
    with pytest.raises(AssertionError, match="blob size"):
        eo.compare_blobs(bad, choice, blks, "size")
    with pytest.raises(AssertionError, match="choice"):
        eo.compare_blobs(blobs(), choice + np.array([0, 1]), blks, "choice")
    # the oracle cut the chosen blob after its size was recorded: equal up to the cut, and only with cut=True
    cut = [dict(b, blobs=[x[:-2] if kb == b["choice"] else x for kb, x in enumerate(b["blobs"])]) for b in blks]
    with pytest.raises(AssertionError, match="blob bytes"):
        eo.compare_blobs(blobs(), choice, cut, "cut")
    assert eo.compare_blobs(blobs(), choice, cut, "cut", cut=True) == len(blks)


def test_shape_streams_are_shared(oracle):
    keep = ("lW", "nW", "block_mode", "pcm", "packet", "tone")
    a = eo.streams_for(oracle, 1, 8000, 0.5, 5, keep, distinct=2)
    b = eo.streams_for(oracle, 1, 8000, 0.5, 2, keep, distinct=2, first=1)
    assert a[0] is a[2] is a[4] is b[1] and a[1] is a[3] is b[0] and a[0] is not a[1]
    assert set(a[0][0]) == set(keep)
