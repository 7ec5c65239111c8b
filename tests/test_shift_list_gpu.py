"""The front end's buffer shift walks a list (csrc/frontend_kernels.hip: fe_decide_one lists the streams whose origin
passes base_max with the round's block, k_fe_shift strides over list x channels, k_fe_flip empties the list).

After every write and every device-built round the streams' origin, parity, fill and live samples
(vbm_debug_frontend_buffers) are held against a numpy restatement of the rule the shift had before the list: a block
moves its stream's window on by bs(W)/4 + bs(nW)/4 samples (lib/block.c:742-759, centerW is half a long block from
the first block on); the origin moves up by as much, and once it would pass base_max the live samples go to the
start of the other buffer and the parity flips.  Whatever was live before a round and is still live after it must be
there bit for bit, at the new origin; the list's count and members are the model's.

The smallest buffers (VBM_FE_BUFFER_BLOCKS=8: base_max is two long blocks) make a stream compact every four or five
1024-sample writes.  Three phases: every stream the same signal in lock step (all compact in one round), writes of
three sizes by stream (mixed rounds), one stream alone (a list of exactly one).  The round that ends every drain
delivers nothing: no stream moves."""
import numpy as np
import pytest
import torch

from tests.signals import burst_signal

pytestmark = pytest.mark.gpu

BUFFER_BLOCKS = 8


def buffers(v, fe, S, ch, stride):
    base, parity, cur = (np.zeros(S, np.int32) for _ in range(3))
    shift = np.zeros(2 + S, np.int32)
    live = np.zeros((S, ch, stride), np.float32)
    rc = v.lib.vbm_debug_frontend_buffers(fe._h, base.ctypes.data, parity.ctypes.data, cur.ctypes.data, shift.ctypes.data,
                                          live.ctypes.data, stride)
    assert rc == 0, rc
    return base, parity, cur, shift, live


def round_movement(v, out, S, bs):
    """samples every stream's window moved on by in the one round of `out`"""
    info, _, nbytes, _ = out
    nb = nbytes.cpu().numpy()
    rec = info.cpu().numpy().view(np.dtype(v.PacketInfo))[:, 0]
    mv = np.zeros(S, np.int64)
    for k in np.flatnonzero(nb != -2):
        pi = rec[k]
        assert mv[pi["stream"]] == 0 and not pi["eos"]
        mv[pi["stream"]] = bs[pi["W"]] // 4 + bs[pi["nW"]] // 4
    return mv


# 2 channels: 70 streams, a tile of 64 and a part of one; mono and 5.1 with odd counts as well
@pytest.mark.parametrize("cls,S", [((2, 44100, 0.5), 70), ((1, 44100, 0.5), 67), ((6, 48000, 0.8), 5)],
                         ids=["2ch", "1ch", "6ch"])
def test_shift_follows_the_old_rule(cuda, monkeypatch, cls, S):
    import vorbis_aotuv_lancer_amd as v
    monkeypatch.setenv("VBM_FE_BUFFER_BLOCKS", str(BUFFER_BLOCKS))
    ch, rate = cls[0], cls[1]
    setup = v.Setup(*cls)
    bs = setup.blocksizes
    assert bs[1] == 2048
    cap, base_max = BUFFER_BLOCKS * bs[1], bs[1] * (BUFFER_BLOCKS // 3)
    enc = v.Encoder(setup, S, max_batch=v.lib.vbm_device_round_lanes(setup._h, S))
    fe = v.FrontEnd(enc)
    assert fe.capacity == cap - 3 * bs[1] - base_max

    # the schedule: (sizes by stream) per write
    lone = 3
    writes = [{s: 1024 for s in range(S)} for _ in range(12)]
    writes += [{s: (512, 1024, 1536)[s % 3] for s in range(S)} for _ in range(12)]
    writes += [{lone: 1024} for _ in range(8)]
    total = max(sum(w.get(s, 0) for w in writes) for s in range(S))
    sig = torch.from_numpy(burst_signal(ch, rate, total, seed=41, period=9000)).to(cuda)
    at = np.zeros(S, np.int64)

    base_m, par_m, cur_m = np.zeros(S, np.int64), np.zeros(S, np.int64), np.full(S, bs[1] // 2, np.int64)
    seen = dict(none=0, all=0, mixed=0, one=0)
    compactions = np.zeros(S, np.int64)
    for w, sizes in enumerate(writes):
        for n in sorted(set(sizes.values())):
            ids = [s for s in sorted(sizes) if sizes[s] == n]
            fe.write_streams(ids, torch.stack([sig[:, at[s]:at[s] + n] for s in ids]).contiguous())
            for s in ids:
                at[s] += n
                cur_m[s] += n
        base, parity, cur, shift, before = buffers(v, fe, S, ch, cap)
        assert np.array_equal(base, base_m) and np.array_equal(parity, par_m) and np.array_equal(cur, cur_m), f"write {w}"
        for r in range(24):
            mv = round_movement(v, fe.encode_rounds_device(nrounds=1), S, bs)
            compact = (mv > 0) & (base_m + mv > base_max)
            par_m = np.where(compact, par_m ^ 1, par_m)
            base_m = np.where(compact, 0, base_m + mv)
            cur_m = cur_m - mv
            compactions += compact
            where = f"write {w} round {r}"
            base, parity, cur, shift, after = buffers(v, fe, S, ch, cap)
            assert np.array_equal(base, base_m), (where, base, base_m)
            assert np.array_equal(parity, par_m), (where, parity, par_m)
            assert np.array_equal(cur, cur_m), (where, cur, cur_m)
            # the list: empty again, and the round's was the model's
            n = int(compact.sum())
            assert shift[0] == 0 and shift[1] == n, (where, shift[:2], n)
            assert sorted(shift[2:2 + n].tolist()) == np.flatnonzero(compact).tolist(), where
            for s in range(S):
                a, b = after[s, :, :cur_m[s]], before[s, :, mv[s]:mv[s] + cur_m[s]]
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{where}: live samples of stream {s} changed"
            before = after
            moved = int((mv > 0).sum())
            seen["none"] += moved == 0
            seen["all"] += n == S
            seen["mixed"] += 0 < n < moved
            seen["one"] += n == 1
            if moved == 0:
                break
        else:
            raise AssertionError(f"write {w}: streams still deliver blocks after 24 rounds")
    fe.device_stats()
    assert fe.refused_writes == 0
    assert min(seen.values()) > 0, seen
    assert compactions.min() >= 2 and compactions[lone] >= 3, compactions
    fe.close()
    enc.close()
    setup.close()
