"""Shared by the shape tests of single kernels (tests/test_tonemask_shapes_gpu.py, tests/test_couple_consts_gpu.py,
tests/test_psy_small_forms_gpu.py): a schedule that hands the oracle block sequences of a few distinct signals
(tests/encode_oracle.py, streams_for) to vbm_analysis_batch in batches of an exact size per block type.

A batch's size is what selects a kernel's tail workgroup, its second tile and so on, so the tests want batches of
exactly B stream-blocks of one type.  B streams are run side by side.  Every call takes the streams whose NEXT block
has the highest block type any stream is waiting with (long before transition before padding before impulse), so the
streams that are ahead wait at the type boundary round a burst until the others arrive: with signals whose bursts
start at the same sample the whole set goes through every type together at least once.  `schedule()` is plain Python
over the oracle's block lists; the tests assert the coverage they rely on."""


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


def run_schedule(enc, cuda, streams, calls, stages, ch, on_call=None):
    """Runs the calls; the named stages and the packets are the oracle's, bit for bit (tests/encode_calls.py,
    run_lockstep: `k` of a failure's label is the call's index)"""
    from tests.encode_calls import run_lockstep
    steps = ((k, mode, ids, ids, [streams[s][i] for s, i in zip(ids, idx)]) for k, (mode, ids, idx) in enumerate(calls))
    run_lockstep(enc, cuda, streams, ch, [s for s in stages if s != "residue"], [s for s in stages if s == "residue"],
                 schedule=steps, on_call=on_call)
