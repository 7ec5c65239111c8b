"""The decoder's entry points share one staging ring (four pinned slots) and one front launch chain.  Fifteen calls
of all five kinds (restart_streams, synthesis_batch, synthesis_runs, synthesis_ranges in several sub-calls,
decode_index_device in two scan launches) enqueued back to back, with no wait between them (every input and output
buffer is made before the first call, and nothing but the calls stands between the first and the last), give bit for
bit what the same calls give on a fresh decoder with a device synchronise after each: no call overwrites a table that
an earlier one has still in flight.  What the calls compute is pinned elsewhere (runs against stepwise, ranges against linear, the
device index against the host's)."""
import numpy as np
import pytest
import torch

from tests.decode_calls import FILL_RANGES, batch_inputs, encoded, runs_inputs
from tests.decode_packets import as_stream

MAX_BATCH = 8                                              # one staging slot: 4 * 8 + 1 ints, 32 streams' first packets
INDEX_STREAMS = 40                                         # more than that: two k_index_scan launches, two slots
CYCLES = 3                                                 # of the five kinds: 15 calls, 9 + 3 * sub-calls ring turns


@pytest.fixture(scope="module")
def material(cuda):
    """about 1 s of stereo q5 from the device encoder -> (v, headers, packets [(bytes, granulepos, eos)])"""
    import vorbis_aotuv_lancer_amd as v
    setup = v.Setup(2, 44100, 0.5)
    pk = encoded(v, setup, 1.0, 77, cuda)
    assert len(pk) >= 40
    return v, v.header_packets(setup), pk


def run_sequence(v, headers, pk, cuda, halfrate, sync):
    """the calls on a fresh decoder and store -> [(name, numpy arrays)] per call, read after one last wait"""
    ds = v.DecodeSetup(headers)
    dec = v.Decoder(ds, 2, MAX_BATCH, halfrate=halfrate)
    failed = (headers[0], -1, 0)                           # a header where audio belongs: ENOTAUDIO, no samples
    store = v.RangeStore(dec, [as_stream(pk), as_stream(pk[:30]), as_stream(pk[:12] + [failed] + pk[12:25])])
    one_packet = runs_inputs([[p] for p in pk[:INDEX_STREAMS]], cuda)[:4]
    first = np.arange(INDEX_STREAMS + 1, dtype=np.int64)
    # every input and output buffer of every call is made here, before the first call, and held to the end: an upload
    # waits for the stream, so the loop below holds decoder calls only
    plan = []
    for c in range(CYCLES):
        a = 5 * c
        *rows, gp, eo = batch_inputs(pk[a:a + 2], cuda)
        runs = [pk[a + 2:a + 4] + [failed] + pk[a + 4:a + 6], pk[a + 1:a + 4]]      # 5 + 3 rows
        windows = ([0, 1, 2, 0], [100 * c, 3000, 4000 + c, 7000], [9000, 9000, 5000, 2000 + c])
        buf = torch.full((4, dec.channels, 9000), FILL_RANGES, dtype=torch.float32, device=cuda)
        row = dec.row
        outs = dict(batch=(torch.zeros((2, dec.channels, row), dtype=torch.float32, device=cuda),
                           torch.zeros(2, dtype=torch.int32, device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda)),
                    runs=(torch.zeros((2, dec.channels, 5 * row), dtype=torch.float32, device=cuda),
                          torch.zeros(2, dtype=torch.int32, device=cuda), torch.zeros(8, dtype=torch.int32, device=cuda),
                          torch.zeros(8, dtype=torch.int32, device=cuda)))
        plan.append((rows, gp, eo, [len(r) for r in runs], runs_inputs(runs, cuda), windows, buf, outs))
    # decode_index_device makes its own outputs: blocks of their sizes are left with torch's allocator, so that it has
    # nothing to ask the device for inside the loop
    spare = [torch.empty(INDEX_STREAMS, dtype=dt, device=cuda) for _ in range(CYCLES)
             for dt in (torch.int32, torch.int32, torch.int32, torch.int64, torch.int64)]
    del spare
    torch.cuda.synchronize()
    calls = []

    def done():
        if sync:
            torch.cuda.synchronize()

    for c, (rows, gp, eo, counts, t, windows, buf, outs) in enumerate(plan):
        dec.restart_streams([c % 2])
        done()
        calls.append(("batch", dec.synthesis_batch([1, 0], *rows, granulepos=gp, eos=eo, out=outs["batch"])))
        done()
        calls.append(("runs", dec.synthesis_runs([1, 0], counts, *t[:2], granulepos=t[2], eos=t[3], out=outs["runs"])))
        done()
        calls.append(("ranges", dec.synthesis_ranges(store, *windows, out=buf)))
        done()
        calls.append(("index", v.decode_index_device(dec, *one_packet, stream_packets=first)))
        done()
    torch.cuda.synchronize()
    res = []
    for name, out in calls:
        out = [o.cpu().numpy() if torch.is_tensor(o) else np.asarray(o) for o in out]
        if name in ("batch", "runs"):                      # pcm [rows, ch, stride] within samples / run_samples [rows]
            out[0] = np.stack([np.where(np.arange(out[0].shape[2]) < n, p, 0) for p, n in zip(out[0], out[1])])
        res.append((name, out))
    del plan
    store.close()
    dec.close()
    ds.close()
    return res


@pytest.mark.gpu
def test_back_to_back_calls_equal_synchronised_calls(cuda, material):
    v, headers, pk = material
    for halfrate in (False, True):
        free = run_sequence(v, headers, pk, cuda, halfrate, sync=False)
        want = run_sequence(v, headers, pk, cuda, halfrate, sync=True)
        assert [n for n, _ in free] == [n for n, _ in want] and len(want) == 4 * CYCLES       # and CYCLES restarts
        for k, ((name, got), (_, ref)) in enumerate(zip(free, want)):
            assert len(got) == len(ref)
            for j, (g, r) in enumerate(zip(got, ref)):
                assert g.dtype == r.dtype and np.array_equal(g, r), f"halfrate {halfrate}: call {k} ({name}), output {j}"
        # the sequence crossed what it is meant to: a failed packet among the runs, ranges of several sub-calls, PCM
        by = {name: out for name, out in want}
        assert (by["runs"][3] != 0).sum() == 1 and by["runs"][1].min() > 0
        assert by["ranges"][1][0] == 9000 and by["ranges"][1].sum() > 15000 and np.any(by["ranges"][0] != FILL_RANGES)
        assert by["index"][4].shape == (INDEX_STREAMS,) and np.all(by["index"][0] == 0)
        assert by["batch"][1].max() > 0 and np.abs(by["batch"][0]).max() > 0
