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

from tests.encode_calls import write_and_drain
from tests.encode_oracle import compare_records, records, walk
from tests.vq_edge_cases import CASES, N

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,ch,rate,q,make", CASES, ids=[c[0] for c in CASES])
def test_edge_signal_matches_oracle(oracle, cuda, name, ch, rate, q, make):
    import vorbis_aotuv_lancer_amd as v
    pcm = make(ch, rate)
    assert pcm.shape == (ch, N) and pcm.dtype == np.float32
    want = records(walk(oracle, ch, rate, q, pcm=pcm, capture=False))
    assert len(want) > 40 and {w[0][1] for w in want} == {0, 1}, "the signal must produce long and short blocks"

    # two streams with the same input (lanes 0 and 1 of a tile), written 1024 samples at a time
    S = 2
    enc = v.Encoder(v.Setup(ch, rate, q), S)
    fe = v.FrontEnd(enc)
    got = [[] for _ in range(S)]
    write_and_drain(fe, cuda, [pcm] * S, got)
    fe.close()
    for s in range(S):
        compare_records(got[s], want, f"stream {s}")
