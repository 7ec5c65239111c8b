"""Host side of the encoder tests: the one oracle stream walk, the block record, the per-block lock-step schedule, the
signals of the kernel shape tests and the comparers.  numpy and tests.orc only, no torch: tests/test_encode_toolkit_cpu.py
pins every function in here on the CPU.  The device side (drivers that call the library) is tests/encode_calls.py."""
import numpy as np

from tests import orc

RECORD_FIELDS = ("lW", "W", "nW", "block_mode", "eos", "granulepos", "packetno")
RECORD_KEEP = ("lW", "W", "nW", "block_mode", "eos", "granulepos", "sequence", "packet")       # walk(keep=): what record() reads
_cache, _setups = {}, {}


def setup_of(oracle, ch, rate, q=None, bitrate=None):
    """the oracle's setup of a class: loaded once"""
    key = (id(oracle), ch, rate, q, tuple(bitrate) if isinstance(bitrate, (tuple, list)) else bitrate)
    if key not in _setups:
        _setups[key] = orc.Setup(oracle, ch, rate, q, bitrate=bitrate)
    return _setups[key]


# ---- the oracle stream walk ------------------------------------------------------------------------------------------
def walk(oracle, ch, rate, q=None, bitrate=None, pcm=None, chunk=1024, finish=True, capture=True, keep=None, key=None,
         on_block=None):
    """The oracle's blocks of one signal -> list of block dicts (tests/orc.py, Stream.blocks).  pcm (ch, n), or with `key` a
    function that makes it (called only when the result is not cached yet; `key` then names the signal alone), is written
    `chunk` samples at a time (None: in one call) and the ready blocks are collected after every write.  finish: the end
    of the stream is declared and the tail blocks collected.  capture=False: no stage vectors, the packets and block
    fields are the same.  keep: the fields a dict is reduced to (those the block has).  on_block(stream, block, ended) is
    called for every block as it comes out; ended: the end of the stream has been declared.  key: the result is computed
    once per session and its arrays are read-only; the cache key is `key` and every argument that changes the result."""
    if key is not None:
        assert on_block is None
        key = (key, ch, rate, q, tuple(bitrate) if isinstance(bitrate, (tuple, list)) else bitrate,
               None if callable(pcm) else pcm.shape[1], chunk, finish, capture, None if keep is None else tuple(keep))
        if key in _cache:
            return _cache[key]
    if callable(pcm):
        pcm = pcm()
    assert pcm.dtype == np.float32 and pcm.shape[0] == ch, (pcm.dtype, pcm.shape)
    st = orc.Stream(setup_of(oracle, ch, rate, q, bitrate))
    if not capture:
        oracle.lib.orc_stream_set_capture(st.v, 0)
    out = []

    def collect(ended=False):
        for b in st.blocks():
            if on_block is not None:
                on_block(st, b, ended)
            out.append(b if keep is None else {k: b[k] for k in keep if k in b})

    for at in range(0, pcm.shape[1], chunk or max(pcm.shape[1], 1)):
        st.write(pcm[:, at:at + chunk] if chunk else pcm)
        collect()
    if finish:
        st.finish()
        collect(True)
    st.close()
    if key is not None:
        for b in out:
            for x in b.values():
                if isinstance(x, np.ndarray):
                    x.flags.writeable = False
        _cache[key] = out
    return out


def record(b, packet=None):
    """((lW, W, nW, block_mode, eos, granulepos, packetno), packet bytes) of an oracle block dict, or of a PacketInfo row
    and its packet"""
    if isinstance(b, dict):
        return (b["lW"], b["W"], b["nW"], b["block_mode"], b["eos"], b["granulepos"], b["sequence"]), b["packet"]
    return (int(b["lW"]), int(b["W"]), int(b["nW"]), int(b["block_mode"]), int(b["eos"]), int(b["granulepos"]),
            int(b["packetno"])), packet


def records(blocks):
    return [record(b) for b in blocks]


# ---- the per-block schedule ------------------------------------------------------------------------------------------
def lockstep(streams, R=1, stop="longest"):
    """Lock step over the block lists `streams`: the k-th block of every stream that has one, one call per block type
    present, in ascending type; stop="shortest" ends at the shortest stream.  Yields (k, block_mode, present, ids, blks):
    present = the signals in the call (ascending), blks = their k-th blocks.  With R replicas there are K * R streams,
    stream s carrying signal s % K: ids = r * K + signal for r < R, so row r of a call holds signal
    present[r % len(present)], the first len(present) rows are the first copies and every call holds all R copies of
    each signal present."""
    K = len(streams)
    for k in range((max if stop == "longest" else min)(len(b) for b in streams)):
        by_mode = {}
        for m, blocks in enumerate(streams):
            if k < len(blocks):
                by_mode.setdefault(blocks[k]["block_mode"], []).append(m)
        for mode, present in sorted(by_mode.items()):
            ids = (np.arange(R, dtype=np.int32)[:, None] * K + np.asarray(present, np.int32)[None, :]).reshape(-1)
            yield k, mode, present, ids, [streams[m][k] for m in present]


# ---- signals of the kernel shape tests (tone mask, couple constants) ----------------------------------------------------
NSAMP, FIRST, SECOND = 26624, 6000, 17000
KINDS = ("silence", "sine", "noise", "twotone")


def shape_signal(kind, variant, ch, rate):
    """Every signal starts with digital silence (the same first blocks for all), begins at sample FIRST and has a
    burst, a step or a second click at sample SECOND."""
    rng = np.random.default_rng(1000 + 16 * variant + KINDS.index(kind))
    pos = np.arange(NSAMP)
    t = pos.astype(np.float64) / rate
    on = pos >= FIRST
    burst = (pos >= SECOND) & (pos < SECOND + 200)
    out = np.zeros((ch, NSAMP), np.float64)
    level = 0.8 ** variant
    for c in range(ch):
        if kind == "silence":
            if c == 0:
                out[c, FIRST] = out[c, SECOND] = 0.9 * level
        elif kind == "sine":
            out[c] = np.where(on, level * np.sin(2 * np.pi * (997.0 + 211.0 * variant) * (c + 1) * t), 0.0)
            out[c] += np.where(burst, 0.6 * rng.uniform(-1, 1, NSAMP), 0.0)
        elif kind == "noise":
            out[c] = np.where(pos >= SECOND, 0.8 * level, np.where(on, 0.02, 0.0)) * rng.uniform(-1, 1, NSAMP)
        else:
            f = 1500.0 * (1.0 + 0.37 * variant)
            x = 0.4 * np.sin(2 * np.pi * f * t) + (0.4 if (variant + c) % 2 == 0 else 0.25) * np.sin(2 * np.pi * f * 2 ** 0.125 * t)
            out[c] = np.where(on, level * x, 0.0) + np.where(burst, 0.6 * rng.uniform(-1, 1, NSAMP), 0.0)
    return out.astype(np.float32)


def distinct_streams(oracle, ch, rate, q, keep, distinct, bitrate=None, make=shape_signal, kinds=KINDS):
    """the oracle's blocks of `distinct` signals make(kind d % 4, variant d // 4), 1024 samples per write, the end not
    declared, reduced to `keep`: computed once"""
    return [walk(oracle, ch, rate, q, bitrate, lambda d=d: make(kinds[d % 4], d // 4, ch, rate), finish=False, keep=keep,
                 key=(make.__name__, d)) for d in range(distinct)]


def streams_for(oracle, ch, rate, q, B, keep, distinct, first=0, **kw):
    """B streams side by side: stream s carries distinct signal (first + s) % distinct"""
    d = distinct_streams(oracle, ch, rate, q, keep, distinct, **kw)
    return [d[(first + s) % distinct] for s in range(B)]


# ---- the comparers (host arrays) -------------------------------------------------------------------------------------
def compare_records(got, want, label):
    """one stream's records from the device against the oracle's: the block sequence first, then every packet"""
    gm, wm = [m for m, _ in got], [m for m, _ in want]
    if gm != wm:
        at = next((i for i, (a, b) in enumerate(zip(gm, wm)) if a != b), min(len(gm), len(wm)))
        raise AssertionError(f"{label}: block sequence differs from the oracle at record {at} of {len(wm)} (got {len(gm)}): "
                             f"{gm[at] if at < len(gm) else None} against {wm[at] if at < len(wm) else None} {RECORD_FIELDS}")
    bad = [i for i in range(len(want)) if got[i][1] != want[i][1]]
    assert not bad, f"{label}: packet {bad[0]} of {len(want)} differs from the oracle ({len(bad)} differ)"


def compare_block_call(got, blks, ch, float_stages, int_stages, res1_channels=(), label=""):
    """The stage rows of one analysis_batch call against the oracle's captures of its blocks `blks`, bit for bit.
    got: stage name -> host array, the rows of the blocks in order.  Float stages are compared as uint32 (so -0.0 is not
    0.0).  `residue` among the int stages leaves out the channels of a type-1 residue (encoded in place, lib/res0.c:372-375:
    after the packet kernel those rows hold the VQ remainder)."""
    for name in tuple(float_stages) + tuple(int_stages):
        want = np.concatenate([np.atleast_1d(b[name]) for b in blks])
        have = np.asarray(got[name])
        assert have.shape == want.shape, (label, name, "shape", have.shape, want.shape)
        if name in float_stages:
            have, want = have.view(np.uint32), want.view(np.uint32)
        if name == "residue" and res1_channels:
            keep = np.array([c not in res1_channels for c in range(ch)] * len(blks))
            have, want = have[keep], want[keep]
        diff = have != want
        if diff.any():
            at = tuple(int(x) for x in np.argwhere(diff)[0])
            raise AssertionError((label, name, "first difference at", at, have[at], want[at], "of", int(diff.sum())))


def compare_packets(packets, nbytes, want, label, zero_tail=False):
    """rows of `packets` (uint8 [rows, max bytes]) and their lengths against the packets in `want` (bytes); zero_tail:
    the row is zero past the packet"""
    assert len(want) == packets.shape[0] == nbytes.shape[0], (label, len(want), packets.shape, nbytes.shape)
    for i, w in enumerate(want):
        assert nbytes[i] == len(w), (label, "packet length", i, int(nbytes[i]), len(w))
        if bytes(packets[i, :nbytes[i]]) != w:
            at = next(k for k in range(len(w)) if packets[i, k] != w[k])
            raise AssertionError((label, "packet bytes", i, "first differing byte", at, "of", len(w)))
        if zero_tail:
            tail = np.flatnonzero(packets[i, nbytes[i]:])
            assert tail.size == 0, (label, "row not zero past the packet", i, "length", int(nbytes[i]), "first byte",
                                    int(nbytes[i] + tail[0]), "value", int(packets[i, nbytes[i] + tail[0]]), "count", int(tail.size))


def compare_blobs(blobs, choice, blks, label, cut=False):
    """managed bitrate: the fifteen packetblobs (host arrays (bytes, lengths)) and the bitrate manager's choice of one
    call against the oracle's.  cut: the oracle cuts the chosen blob in place (oggpack_writetrunc, to whole bytes) after
    its size was recorded, the device cuts the packet it hands out; the blob is then compared up to the cut.  -> blobs cut"""
    ncut = 0
    for kb, (bp, bn) in enumerate(blobs):
        for i, b in enumerate(blks):
            assert bn[i] == b["blob_bytes"][kb], (label, "blob size", kb, i, int(bn[i]), b["blob_bytes"][kb])
            have, want = bytes(bp[i, :bn[i]]), b["blobs"][kb]
            if cut and kb == b["choice"] and len(want) < bn[i]:
                have = have[:len(want)]
                ncut += 1
            assert have == want, (label, "blob bytes", kb, i)
    for i, b in enumerate(blks):
        assert choice[i] == b["choice"], (label, "choice", i, int(choice[i]), b["choice"])
    return ncut
