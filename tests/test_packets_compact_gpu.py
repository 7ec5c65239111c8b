"""vbm_packets_compact (k_compact_scan + k_compact_copy, csrc/util_kernels.hip) against numpy.

The copy-out of a host consumer and of the drop-in shim: rows [n][M] with lengths -> one byte run, packet k at the
exclusive prefix sum of the lengths rounded up to 4, offsets[n] = bytes used.  The scan is one workgroup that carries a
running total across chunks of 1024 entries, the copy one wavefront per row, four rows per workgroup: n sits on, below
and above 64, 1024 and 2048, and 5000 runs five chunks.  Lengths come from the edges of the word rounding and of the row
(negative ones count as 0: -2 is an empty lane of a device-built round, -1 a packet that outgrew its row); values above
M are left out for M = 8, the kernels read the row and nothing says how long it is.  The pad bytes of a packet's last
word are the row's own, nothing past offsets[n] is written."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000]
MS = [8, 4096]
FILL = 0xA5
VBM_OK, VBM_EINVAL = 0, -131         # include/vorbis_mi355x.h


def length_vectors(n, M, rng):
    pool = np.array(sorted({l for l in (-2, -1, 0, 1, 2, 3, 4, 5, 255, 256, M - 1, M) if l <= M}), np.int32)
    return {"mixed": rng.choice(pool, size=n).astype(np.int32), "holes": np.full(n, -2, np.int32),
            "empty": np.zeros(n, np.int32), "full": np.full(n, M, np.int32)}


def compact(v, rows, lens, n, M, out, off):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return v.lib.vbm_packets_compact(rows.data_ptr() if rows is not None else None, lens.data_ptr() if lens is not None else None,
                                     n, M, out.data_ptr() if out is not None else None,
                                     off.data_ptr() if off is not None else None, st)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", NS)
def test_compact_against_numpy(cuda, n, M):
    import vorbis_aotuv_lancer_amd as v
    rng = np.random.default_rng(1000 * n + M)
    rows_h = rng.integers(0, 256, size=(n, M), dtype=np.uint8)          # random over the whole width, pad bytes included
    rows = torch.from_numpy(rows_h).to(cuda)
    for name, lens_h in length_vectors(n, M, rng).items():
        lens = torch.from_numpy(lens_h).to(cuda)
        out = torch.full((n * M + 64,), FILL, dtype=torch.uint8, device=cuda)
        off = torch.full(((n + 1) * 8,), FILL, dtype=torch.uint8, device=cuda).view(torch.int64)
        assert compact(v, rows, lens, n, M, out, off) == VBM_OK
        got_off, got = off.cpu().numpy(), out.cpu().numpy()
        pad = (np.maximum(lens_h, 0).astype(np.int64) + 3) & ~3
        want_off = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
        assert got_off.dtype == np.int64 and np.array_equal(got_off, want_off), \
            f"{name}: offsets differ first at {int(np.flatnonzero(got_off != want_off)[0])} of {n + 1}"
        total = int(want_off[n])
        want = np.full(n * M + 64, FILL, np.uint8)                        # (every byte past offsets[n] keeps the fill)
        keep = np.arange(M)[None, :] < pad[:, None]
        want[:total] = rows_h[keep]                                       # row-major: packet k at want_off[k], pad(l) bytes
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}: {bad.size} bytes differ, first at {int(bad[0])} (offsets[n] = {total})"


def test_compact_argument_checks(cuda):
    import vorbis_aotuv_lancer_amd as v
    n, M = 8, 16
    buf = torch.zeros((n * M + 8,), dtype=torch.uint8, device=cuda)
    out = torch.zeros((n * M + 8,), dtype=torch.uint8, device=cuda)
    lens = torch.full((n,), 5, dtype=torch.int32, device=cuda)
    off = torch.zeros((n + 1,), dtype=torch.int64, device=cuda)
    assert compact(v, buf, lens, n, M, out, off) == VBM_OK
    assert compact(v, buf[1:], lens, n, M, out, off) == VBM_EINVAL          # misaligned rows
    assert compact(v, buf[2:], lens, n, M, out, off) == VBM_EINVAL
    assert compact(v, buf, lens, n, M, out[1:], off) == VBM_EINVAL          # misaligned run
    assert compact(v, buf, lens, n, M, out[3:], off) == VBM_EINVAL
    for bad_M in (0, -4, 1, 6, 15, 17):
        assert compact(v, buf, lens, n, bad_M, out, off) == VBM_EINVAL
    assert compact(v, buf, lens, -1, M, out, off) == VBM_EINVAL
    assert compact(v, None, lens, n, M, out, off) == VBM_EINVAL
    assert compact(v, buf, None, n, M, out, off) == VBM_EINVAL
    assert compact(v, buf, lens, n, M, None, off) == VBM_EINVAL
    assert compact(v, buf, lens, n, M, out, None) == VBM_EINVAL
    torch.cuda.synchronize()


def test_compact_no_rows(cuda):
    """n == 0: offsets[0] = 0 is written (offsets[n] = bytes used, as for every other n), nothing else is touched and
    the other pointers may be NULL; offsets itself may not"""
    import vorbis_aotuv_lancer_amd as v
    out = torch.full((64,), FILL, dtype=torch.uint8, device=cuda)
    off = torch.full((2,), -1, dtype=torch.int64, device=cuda)
    assert compact(v, None, None, 0, 4096, out, off) == VBM_OK
    assert off.cpu().tolist() == [0, -1]
    assert bool((out == FILL).all())
    off.fill_(-1)
    assert compact(v, None, None, 0, 4096, None, off) == VBM_OK
    assert off.cpu().tolist() == [0, -1]
    assert compact(v, None, None, 0, 4096, out, None) == VBM_EINVAL
    assert compact(v, None, None, 0, 6, out, off) == VBM_EINVAL
