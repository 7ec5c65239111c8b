"""The reference's OWN test input on the device: test/util.c:29-45 gen_windowed_sine (2048 samples: a Hann-windowed
sine of period 32 and peak 0.95, then 1024 zeros), written in one piece to every channel and followed at once by
the end of the stream (test/write_read.c:85-99) — start-of-stream extrapolation, block switching and the
end-of-stream extrapolation of an undrained buffer within seven blocks.  For every (channels, rate) of the
reference's matrix (test/test.c:38-57: 1..8 channels x {44100, 48000, 32000, 22050, 16000, 96000} Hz) that has a
shipped mode pack, at the pack's quality: block sequence and packets against the oracle, through the batched front
end and through the reference's own entry points (include/vorbis_compat.h)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import compat
from tests.decode_packets import matrix_classes
from tests.encode_calls import drain
from tests.encode_oracle import compare_records, records, walk
from tests.signals import gen_windowed_sine

pytestmark = pytest.mark.gpu


def test_matrix_is_not_empty():
    cl = matrix_classes()
    assert len(cl) >= 20 and {c[0] for c in cl} == {1, 2, 3, 4, 5, 6, 7, 8} and 96000 in {c[1] for c in cl}


@pytest.mark.parametrize("ch,rate,q", matrix_classes())
def test_windowed_sine_then_eos(oracle, cuda, ch, rate, q):
    import vorbis_aotuv_lancer_amd as v
    sine = gen_windowed_sine()
    pcm = np.repeat(sine[None, :], ch, axis=0)                # the same data on every channel (write_read.c:88-92)
    want = records(walk(oracle, ch, rate, q, pcm=pcm, chunk=None, capture=False))
    assert want and want[-1][0][4] == 1 and want[-1][0][5] == 2048      # e_o_s, last granule = samples written

    # batched front end: S = 3 streams with the same input, end declared before the first round
    S = 3
    enc = v.Encoder(v.Setup(ch, rate, q), S)
    fe = v.FrontEnd(enc)
    fe.write(torch.from_numpy(np.repeat(pcm[None], S, axis=0)).to(cuda))
    fe.finish()
    got = [[] for _ in range(S)]
    drain(fe, got)
    for s in range(S):
        compare_records(got[s], want, f"stream {s}")
    fe.close()

    # the reference's own call sequence (test/write_read.c:85-115); its packets carry no block type
    dll = compat.bind(C.CDLL(v.COMPAT_LIB_PATH))
    st = compat.Stream(dll, ch, rate, q)
    assert st.write(pcm) == 0
    assert st.finish() == 0
    assert st.drain() == [(m[:3] + m[4:], p) for m, p in want]
    st.close()
