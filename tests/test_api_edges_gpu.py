"""Edge cases of the C ABI on the device: argument errors follow the reference's conventions
(OV_EINVAL = VBM_EINVAL, nothing is launched), empty batches are no-ops, digital silence takes the
"floor unused" path (floor1_fit returns NULL, lib/floor1.c:641-644; one zero bit per channel,
lib/floor1.c:969-972) exactly as in the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.encode_calls import collect_device, drain
from tests.encode_oracle import records, walk

pytestmark = pytest.mark.gpu
VBM_EINVAL = -131


def test_analysis_batch_argument_errors(cuda):
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    enc = v.Encoder(v.Setup(2, 44100, 0.5), 8)
    pcm = torch.zeros((4, 2, 2048), device=cuda)
    pk = torch.empty((4, enc.max_packet_bytes), dtype=torch.uint8, device=cuda)
    nb = torch.empty((4,), dtype=torch.int32, device=cuda)
    ids = np.arange(4, dtype=np.int32)
    fl = np.full(4, 3, np.uint8)

    def call(mode=3, n=4, ids_=ids, pcm_ptr=None, pk_ptr=None):
        return lib.vbm_analysis_batch(enc._h, mode, n, ids_.ctypes.data, fl.ctypes.data,
                                      pcm.data_ptr() if pcm_ptr is None else pcm_ptr,
                                      pk.data_ptr() if pk_ptr is None else pk_ptr, nb.data_ptr(), None)
    assert call() == 0
    assert call(mode=4) == VBM_EINVAL and call(mode=-1) == VBM_EINVAL
    assert call(n=9) == VBM_EINVAL                                  # more blocks than the encoder was created for
    assert call(n=0) == 0                                           # empty batch: no-op
    assert call(ids_=np.array([0, 1, 2, 8], np.int32)) == VBM_EINVAL  # stream id out of range
    assert call(ids_=np.array([0, 1, 2, 1], np.int32)) == VBM_EINVAL  # a stream twice in one batch
    assert call(pcm_ptr=pcm.data_ptr() + 4) == VBM_EINVAL           # PCM must be 16-byte aligned
    assert call(pk_ptr=pk.data_ptr() + 1) == VBM_EINVAL             # packets must be 4-byte aligned
    assert lib.vbm_analysis_batch(None, 3, 4, ids.ctypes.data, fl.ctypes.data, pcm.data_ptr(), pk.data_ptr(),
                                  nb.data_ptr(), None) == VBM_EINVAL
    with pytest.raises(ValueError):
        enc.analysis_batch(3, ids, fl, pcm[:, :, :1024].contiguous())   # wrong block size for the block type


def test_frontend_write_errors(cuda):
    import vorbis_aotuv_lancer_amd as v
    from vorbis_aotuv_lancer_amd._lib import lib
    enc = v.Encoder(v.Setup(2, 44100, 0.5), 3)
    fe = v.FrontEnd(enc)
    chunk = torch.zeros((3, 2, 1024), device=cuda)
    assert lib.vbm_frontend_write(fe._h, chunk.data_ptr(), 0, None) == VBM_EINVAL
    assert lib.vbm_frontend_write(fe._h, chunk.data_ptr(), fe.capacity, None) == VBM_EINVAL  # can never fit the buffer
    ids = np.array([1, 1], np.int32)                                # a stream once per call
    assert lib.vbm_frontend_write_streams(fe._h, ids.ctypes.data, 2, chunk.data_ptr(), 1024, None) == VBM_EINVAL
    # without draining, the buffers fill up: the write that would overrun is refused (lib/block.c:540-541)
    refused = False
    for _ in range(fe.capacity // 1024 + 2):
        rc = lib.vbm_frontend_write(fe._h, chunk.data_ptr(), 1024, None)
        if rc == VBM_EINVAL:
            refused = True
            break
        assert rc == 0
    assert refused and fe.max_buffered <= fe.capacity
    got = [[] for _ in range(3)]
    drain(fe, got)                                                   # draining makes room again
    assert lib.vbm_frontend_write(fe._h, chunk.data_ptr(), 1024, None) == 0
    drain(fe, got)
    fe.finish()
    assert lib.vbm_frontend_write(fe._h, chunk.data_ptr(), 1024, None) == VBM_EINVAL     # write after finish
    assert lib.vbm_frontend_finish(fe._h, np.array([0], np.int32).ctypes.data, 1, None) == VBM_EINVAL   # finished twice


def test_device_guard_refuses_oversized_writes(oracle, cuda):
    """The kernels' own guard (f.overflow = device_stats()[5] = FrontEnd.refused_writes), on all three intake paths.
    After a device-built round the host mirrors are stale and the host check steps aside, so a write of twice the
    front end's capacity (more than a channel's whole buffer, whatever its fill) reaches the device: every listed
    stream is counted as refused, no sample is taken, and the streams go on to the oracle's packets for the signal
    without the refused samples."""
    import vorbis_aotuv_lancer_amd as v
    from tests.signals import synth_signal
    S, ch, n, before = 3, 2, 14 * 1024, 4
    sigs = [synth_signal(ch, 44100, n, seed=880 + s) for s in range(S)]
    want = [records(walk(oracle, ch, 44100, 0.5, pcm=sig, capture=False)) for sig in sigs]
    setup = v.Setup(ch, 44100, 0.5)
    enc = v.Encoder(setup, S, max_batch=v.lib.vbm_device_round_lanes(setup._h, S))
    fe = v.FrontEnd(enc)
    got = [[] for _ in range(S)]
    allp = torch.from_numpy(np.stack(sigs)).to(cuda)
    for at in range(0, before * 1024, 1024):
        fe.write(allp[:, :, at:at + 1024].contiguous())
    collect_device(got, fe, fe.encode_rounds_device(nrounds=2))     # the host mirrors are stale from here on
    fe.device_stats()
    assert fe.refused_writes == 0

    big = 2 * fe.capacity
    zeros = torch.zeros((S, ch, big), device=cuda)
    rose = []
    for write in (lambda: fe.write(zeros), lambda: fe.write_streams([0], zeros[:1]),
                  lambda: fe.write_ragged([0], zeros[:1], [0], [big])):
        at0 = fe.refused_writes
        write()
        fe.device_stats()
        rose.append(fe.refused_writes - at0)
    assert rose == [S, 1, 1]
    # what every stream holds: the half long block it starts with and the samples written, less what its blocks so far
    # moved its window on by (a quarter of the block's own size and a quarter of the next one's, lib/block.c:742-759)
    bs = setup.blocksizes
    held = [bs[1] // 2 + before * 1024 - sum(bs[m[1]] // 4 + bs[m[2]] // 4 for m, _ in got[s]) for s in range(S)]
    assert fe.max_buffered == max(held)

    drain(fe, got)
    for at in range(before * 1024, n, 1024):
        fe.write(allp[:, :, at:at + 1024].contiguous())
        drain(fe, got)
    fe.finish()
    drain(fe, got)
    for s in range(S):
        assert got[s] == want[s], f"stream {s} differs from the oracle"
    fe.device_stats()
    assert fe.refused_writes == S + 2


@pytest.mark.parametrize("ch,rate,q", [(2, 44100, 0.5), (6, 48000, 0.8)])
def test_digital_silence_and_near_silence(oracle, cuda, ch, rate, q):
    """stream 0: exact zeros; stream 1: 1e-6 noise; stream 2: silence, then a click, then silence"""
    import vorbis_aotuv_lancer_amd as v
    n = 40 * 1024
    rng = np.random.default_rng(3)
    sigs = [np.zeros((ch, n), np.float32), (1e-6 * rng.standard_normal((ch, n))).astype(np.float32),
            np.zeros((ch, n), np.float32)]
    sigs[2][:, 20000:20003] = 0.9
    want = [records(walk(oracle, ch, rate, q, pcm=sig, capture=False)) for sig in sigs]
    enc = v.Encoder(v.Setup(ch, rate, q), 3)
    fe = v.FrontEnd(enc)
    got = [[] for _ in range(3)]
    allp = torch.from_numpy(np.stack(sigs)).to(cuda)
    for at in range(0, n, 1024):
        fe.write(allp[:, :, at:at + 1024].contiguous())
        drain(fe, got)
    fe.finish()
    drain(fe, got)
    for s in range(3):
        assert got[s] == want[s], f"stream {s} differs from the oracle"
    # exact zeros: every channel's floor is unused -> 1 type bit + mode/window bits + one 0 bit per channel
    assert max(len(p) for _, p in got[0]) <= 2
