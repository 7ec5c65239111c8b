"""Walk through every scheduler of the encoder once (run under rocprofv3 from the root of the tree to trace)."""
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import vorbis_aotuv_lancer_amd as v
from tests.signals import burst_signal

CH, RATE, Q, S, K = 2, 44100, 0.5, 2048, 8
MANAGED = (144000, 128000, 112000)
cuda = torch.device("cuda:0")
NCH = 12
sigs = [burst_signal(CH, RATE, NCH * 1024, seed=70 + k, period=6000, level=1.0 if k % 3 else 0.05) for k in range(K)]
base = torch.from_numpy(np.stack(sigs)).to(cuda)


def chunk(c):
    return base[:, :, c * 1024:(c + 1) * 1024].repeat(S // K, 1, 1).contiguous()


closers = []


def batches(setup):
    g = torch.Generator(device=cuda).manual_seed(3)
    ids = np.arange(S, dtype=np.int32)
    fl = np.full(S, 3, np.uint8)
    blocks = [(0.4 * (torch.rand((S, CH, 2048), generator=g, device=cuda) - 0.5)).contiguous() for _ in range(3)]
    enc = v.Encoder(setup, S)
    closers.append(enc)
    back = torch.cuda.Stream(device=cuda)
    for nsub, two in ((1, False), (3, False), (3, True)):
        enc.set_sub_batches(nsub)
        for k in range(3):
            out = (torch.empty((S, enc.max_packet_bytes), dtype=torch.uint8, device=cuda),
                   torch.empty((S,), dtype=torch.int32, device=cuda))
            enc.analysis_batch(3, ids, fl, blocks[k], back_stream=back if two else None, out=out)
        torch.cuda.synchronize()
    enc.reset()
    torch.cuda.synchronize()


def host_rounds(setup, ncalls):
    enc = v.Encoder(setup, S)
    fe = v.FrontEnd(enc)
    closers.extend([fe, enc])
    c = 0
    for _ in range(ncalls):          # encode_round, joined
        fe.write(chunk(c)); c += 1
        while len(fe.encode_round()[0]):
            pass
    for lazy in (False, True):
        for _ in range(ncalls):
            fe.write(chunk(c)); c += 1
            while fe.encode_rounds(min_rounds=64, max_rounds=4, lazy=lazy)[3]:
                pass
    fe.restart_streams(np.arange(0, S, 2, dtype=np.int32))      # rounds of the lazy calls are pending
    fe.write(chunk(c)); c += 1
    while fe.encode_rounds(min_rounds=64, max_rounds=4, lazy=True)[3]:
        pass
    fe.join()
    torch.cuda.synchronize()
    fe.reset()
    enc.reset()
    fe.write(chunk(0))
    while len(fe.encode_round()[0]):
        pass
    torch.cuda.synchronize()


def device_rounds(setup, ncalls, profile_at=None):
    os.environ["VBM_WORKSPACES"] = "2"
    enc = v.Encoder(setup, S, max_batch=v.lib.vbm_device_round_lanes(setup._h, S))
    fe = v.FrontEnd(enc)
    closers.extend([fe, enc])
    del os.environ["VBM_WORKSPACES"]
    consumer = torch.cuda.Stream(device=cuda)
    for c in range(ncalls):
        if profile_at and c == profile_at[0]:
            enc.profile_begin(4)
        fe.write(chunk(c))
        fe.encode_rounds_device(nrounds=2, lazy=2)
        fe.join(consumer)
        consumer.synchronize()
        if profile_at and c == profile_at[1]:
            enc.profile_end()
    torch.cuda.synchronize()


vbr = v.Setup(CH, RATE, Q)
man = v.Setup(CH, RATE, bitrate=MANAGED)
batches(vbr)
host_rounds(vbr, 2)
device_rounds(vbr, 7)
device_rounds(vbr, 10, profile_at=(6, 7))
host_rounds(man, 2)
device_rounds(man, 2)
torch.cuda.synchronize()
torch.cuda.mem_get_info()          # (hipMemGetInfo: marks the start of the teardown in the trace)
for obj in closers:
    obj.close()
torch.cuda.synchronize()
print("script done")
