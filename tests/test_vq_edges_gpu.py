"""Edges of the back half that the other fixtures may not reach, whole streams through the batched front end,
every packet byte for byte against the oracle:

* the M6 table of couple/quantise (`k_couple_m6stats` -> `k_couple_fast`): a stereo pair with one silent channel
  (one `nonzero` flag clear: the silent channel contributes res = 0) and a pair that is silent on both channels
  for part of the signal (both flags clear: no value, -1 in the table, next to partitions that have one);
* the residue search (`vq_search.h`, `k_res_vq`): a full-scale square wave and clipped noise at q0.1 and q1.0,
  stereo and mono — the largest residue values these packs were found to meet (up to 1368) and books of every
  dimension in use (1, 2, 4, 5, 8), lanes of one wavefront on different books;
* a 5.1 pack: three residue submaps with different channel counts, coupled and uncoupled (`res_view`).

How far the signals reach was counted in a scratch build of the oracle with counters in orc_book_besterror (not
part of the repository), over exactly these inputs ("Residue search: which paths the tests reach"):
0.7 M vectors, NONE of them on a lattice point without a codeword (the exhaustive search) or with a numerator of
2^23 and more (the integer division) — no audio input was found that gets there.  Those two paths are checked by
tests/test_vq_search_cpu.py on the host instead.
"""
import numpy as np
import pytest
import torch

from tests import orc
from tests.vq_edge_cases import CASES, N

pytestmark = pytest.mark.gpu

def oracle_packets(oracle, ch, rate, q, pcm):
    st = orc.Stream(orc.Setup(oracle, ch, rate, q))
    oracle.lib.orc_stream_set_capture(st.v, 0)
    want = []
    for at in list(range(0, pcm.shape[1], 1024)) + [None]:
        if at is None:
            st.finish()
        else:
            st.write(pcm[:, at:at + 1024])
        want += [((b["lW"], b["W"], b["nW"], b["eos"], b["granulepos"], b["sequence"]), b["packet"]) for b in st.blocks()]
    st.close()
    return want


@pytest.mark.parametrize("name,ch,rate,q,make", CASES, ids=[c[0] for c in CASES])
def test_edge_signal_matches_oracle(oracle, cuda, name, ch, rate, q, make):
    import vorbis_aotuv_lancer_amd as v
    pcm = make(ch, rate)
    assert pcm.shape == (ch, N) and pcm.dtype == np.float32
    want = oracle_packets(oracle, ch, rate, q, pcm)
    assert len(want) > 40 and {w[0][1] for w in want} == {0, 1}, "the signal must produce long and short blocks"

    # two streams with the same input (lanes 0 and 1 of a tile), written 1024 samples at a time
    S = 2
    enc = v.Encoder(v.Setup(ch, rate, q), S)
    fe = v.FrontEnd(enc)
    got = [[] for _ in range(S)]

    def drain():
        while True:
            info, packets, nbytes = fe.encode_round()
            if len(info) == 0:
                return
            packets, nbytes = packets.cpu().numpy(), nbytes.cpu().numpy()
            for k, pi in enumerate(info):
                got[int(pi["stream"])].append(((int(pi["lW"]), int(pi["W"]), int(pi["nW"]), int(pi["eos"]),
                                                int(pi["granulepos"]), int(pi["packetno"])), bytes(packets[k, :nbytes[k]])))

    allp = torch.from_numpy(np.repeat(pcm[None], S, axis=0)).to(cuda)
    for at in range(0, N, 1024):
        fe.write(allp[:, :, at:at + 1024].contiguous())
        drain()
    fe.finish()
    drain()
    fe.close()
    for s in range(S):
        assert len(got[s]) == len(want), f"stream {s}: {len(got[s])} packets, the oracle has {len(want)}"
        for k, (g, w) in enumerate(zip(got[s], want)):
            assert g[0] == w[0], f"stream {s} packet {k}: block {g[0]} against the oracle's {w[0]}"
            assert g[1] == w[1], f"stream {s} packet {k} (W={w[0][1]}): {len(g[1])} bytes differ from the oracle's {len(w[1])}"
