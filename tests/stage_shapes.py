"""Shared by the shape tests of single kernels (tests/test_tonemask_shapes_gpu.py, tests/test_couple_consts_gpu.py):
oracle block sequences of a few distinct signals, and a schedule that hands them to vbm_analysis_batch in batches of
an exact size per block type.

A batch's size is what selects a kernel's tail workgroup, its second tile and so on, so the tests want batches of
exactly B stream-blocks of one type.  B streams are run side by side.  Every call takes the streams whose NEXT block
has the highest block type any stream is waiting with (long before transition before padding before impulse), so the
streams that are ahead wait at the type boundary round a burst until the others arrive: with signals whose bursts
start at the same sample the whole set goes through every type together at least once.  `schedule()` is plain Python
over the oracle's block lists; the tests assert the coverage they rely on."""
import numpy as np

from tests import orc

KEEP = ("lW", "nW", "block_mode", "pcm", "packet", "tone", "residue")


def oracle_stream_blocks(oracle, ch, rate, q, sig, bitrate=None, keep=KEEP):
    """all blocks of one signal (writes of 1024 samples, then end of stream), reduced to the fields in `keep`"""
    setup = orc.Setup(oracle, ch, rate, q, bitrate=bitrate)
    st = orc.Stream(setup)
    out = []
    for i in range(0, sig.shape[1], 1024):
        st.write(sig[:, i:i + 1024])
        out.extend({k: b[k] for k in keep if k in b} for b in st.blocks())
    st.close()
    return out


def schedule(streams):
    """streams: list of block lists.  Returns the calls [(block_mode, [stream ids], [block index of each])]."""
    cur = [0] * len(streams)
    calls = []
    while True:
        ready = {}
        for s, blocks in enumerate(streams):
            if cur[s] < len(blocks):
                ready.setdefault(blocks[cur[s]]["block_mode"], []).append(s)
        if not ready:
            return calls
        mode = max(ready)
        ids = ready[mode]
        calls.append((mode, ids, [cur[s] for s in ids]))
        for s in ids:
            cur[s] += 1


def full_batches(calls, nstreams):
    """block types that some call ran with all `nstreams` streams in the batch"""
    return {mode for mode, ids, _ in calls if len(ids) == nstreams}


def run_schedule(enc, cuda, streams, calls, stages, on_batch=None):
    """Runs the calls; compares the named float / int stages and the packets with the oracle's, bit for bit.
    Returns the list of mismatches (call index, block type, batch size, what, where)."""
    import torch
    bad = []
    for k, (mode, ids, idx) in enumerate(calls):
        blks = [streams[s][i] for s, i in zip(ids, idx)]
        pcm = torch.from_numpy(np.stack([b["pcm"] for b in blks])).to(cuda)
        packets, nbytes = enc.analysis_batch(mode, ids, [b["lW"] | (b["nW"] << 1) for b in blks], pcm)
        for name in stages:
            got = enc.fetch(name).cpu().numpy().view(np.uint32)
            ref = np.concatenate([b[name] for b in blks]).view(np.uint32)
            if not np.array_equal(got, ref):
                bad.append((k, mode, len(ids), name, tuple(np.argwhere(got != ref)[0])))
        if on_batch is not None:
            on_batch(k, mode, ids, blks, bad)
        packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
        for i, b in enumerate(blks):
            if nbytes[i] != len(b["packet"]) or bytes(packets[i, :max(nbytes[i], 0)]) != b["packet"]:
                bad.append((k, mode, len(ids), "packet", (ids[i], int(nbytes[i]), len(b["packet"]))))
        if bad:
            break
    return bad
