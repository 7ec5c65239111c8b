"""Oracle MDCT / window against first principles (CPU only).

The reference ships no golden vectors for mdct_forward; the restatement is
pinned end-to-end by the packet goldens (tests/test_oracle_packets.py).  Here it is
checked against the transform's definition in float64 and for internal consistency.  The scalar inverse
(orc_mdct_backward), the yardstick the device decoder's PCM is compared with bit for bit, is pinned by no output of the
reference at all: it is checked here against the float64 definition, on unit impulses, for its exact properties and
through the TDAC round trip."""
import numpy as np
import pytest


def mdct_definition(x):
    n = x.shape[-1]
    j = np.arange(n)[None, :]
    k = np.arange(n // 2)[:, None]
    basis = np.cos(2 * np.pi / n * (j + .5 + n / 4) * (k + .5))
    return (4.0 / n) * (basis @ x.astype(np.float64).T).T


@pytest.mark.parametrize("n", [64, 256, 512, 2048])
def test_oracle_mdct_matches_definition(oracle, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((4, n)).astype(np.float32)
    got = oracle.mdct_forward(x)
    ref = mdct_definition(x)
    # float32 butterflies: error grows ~ log2(n) * eps * |x|
    assert np.abs(got - ref).max() < 4e-7 * np.sqrt(n)


@pytest.mark.parametrize("n", [256, 2048])
def test_oracle_mdct_trig_table(oracle, n):
    T = oracle.mdct_trig(n)
    i = np.arange(n // 4)
    assert np.array_equal(T[0:n // 2:2], np.cos(np.pi / n * 4 * i).astype(np.float32))
    assert np.array_equal(T[n // 2 + 1:n:2], np.sin(np.pi / (2 * n) * (2 * i + 1)).astype(np.float32))


def test_oracle_mdct_linearity_and_zero(oracle):
    n = 2048
    rng = np.random.default_rng(7)
    x = rng.standard_normal(n).astype(np.float32)
    assert np.all(oracle.mdct_forward(np.zeros(n, np.float32)) == 0)
    # exact power-of-two scaling commutes with every float op in the network
    assert np.array_equal(oracle.mdct_forward(x * 4.0), oracle.mdct_forward(x) * 4.0)


def test_oracle_window_regions(oracle):
    from vorbis_aotuv_lancer_amd.tables import window_table
    wl, ws = window_table(2048), window_table(256)
    x = np.ones(2048, np.float32)
    # long block between a short and a long neighbour (lW=0, nW=1): lib/window.c:2145-2152
    y = oracle.apply_window(x, ws, wl)
    assert np.all(y[:448] == 0) and np.array_equal(y[448:576], ws) and np.all(y[576:1024] == 1)
    assert np.array_equal(y[1024:], wl[::-1])
    y = oracle.apply_window(x, wl, ws)
    assert np.all(y[1024:1472] == 1) and np.array_equal(y[1472:1600], ws[::-1]) and np.all(y[1600:] == 0)


# ---- the scalar inverse (orc_mdct_backward): the yardstick of the device decoder's PCM ---------------------------------
def imdct_basis(n):
    """float64 mdct_backward as tests/decode_calls.py's imdct64 defines it: out = B X with
    B[t, k] = cos(2 pi / n (t + 1/2 + n/4)(k + 1/2)); the forward above is 4/n B^T x"""
    t = np.arange(n)[:, None]
    k = np.arange(n // 2)[None, :]
    return np.cos(2 * np.pi / n * (t + .5 + n / 4) * (k + .5))


# max |orc_mdct_backward - float64 definition| / peak of the float64 output, measured on the CPU with the spectra of
# test_oracle_imdct_matches_definition (4 rows of standard normal bins, seed 100 + n).  The tests assert 4 x these.
IMDCT_MEASURED = {128: 1.43e-07, 256: 1.54e-07, 512: 1.43e-07, 1024: 1.61e-07, 2048: 1.75e-07, 4096: 2.03e-07}
IMDCT_SIZES = sorted(IMDCT_MEASURED)


def imdct_error(oracle, n, X):
    """X: [rows, n/2] float32 -> (max |oracle - definition|, peak of the definition's output)"""
    ref = X.astype(np.float64) @ imdct_basis(n).T
    got = oracle.mdct_backward(X)
    assert got.dtype == np.float32 and got.shape == ref.shape
    return float(np.abs(got - ref).max()), float(np.abs(ref).max())


@pytest.mark.parametrize("n", IMDCT_SIZES)
def test_oracle_imdct_matches_definition(oracle, n):
    """Seeded normal spectra against the float64 definition.  Measured max |error| / peak:
    n = 128: 1.43e-07, 256: 1.54e-07, 512: 1.43e-07, 1024: 1.61e-07, 2048: 1.75e-07, 4096: 2.03e-07 (eleven other seeds: 0.6 to 1.3 x
    these); the bound is 4 x the measured value, never a figure from the device."""
    X = np.random.default_rng(100 + n).standard_normal((4, n // 2)).astype(np.float32)
    err, peak = imdct_error(oracle, n, X)
    print(f"\nn = {n}: max |error| / peak = {err / peak:.3g}")
    assert err <= 4 * IMDCT_MEASURED[n] * peak, (err / peak, IMDCT_MEASURED[n])


@pytest.mark.parametrize("n", IMDCT_SIZES)
def test_oracle_imdct_exact_properties(oracle, n):
    X = np.random.default_rng(200 + n).standard_normal((3, n // 2)).astype(np.float32)
    assert np.all(oracle.mdct_backward(np.zeros(n // 2, np.float32)) == 0)
    y = oracle.mdct_backward(X)
    # a power of two commutes with every rounding of the network
    assert np.array_equal(oracle.mdct_backward(X * np.float32(4.0)), y * np.float32(4.0))
    # the unfold (lib/mdct.c:1599-1625): odd about n/4, even about 3n/4, for every u
    u = np.arange(n // 4)
    assert np.all(y[:, n // 4 - 1 - u] == -y[:, n // 4 + u])
    assert np.all(y[:, 3 * n // 4 - 1 - u] == y[:, 3 * n // 4 + u])
    assert np.abs(y).max() > 1                                    # not vacuous


@pytest.mark.parametrize("n", [128, 4096])
def test_oracle_imdct_unit_impulses(oracle, n):
    """a unit impulse at every bin gives that bin's float64 basis vector (peak 1) within the bound of n: a wrong trig
    index shows at its bin.  Measured: n = 128: 2.32e-07, n = 4096: 4.36e-07."""
    B = imdct_basis(n)
    got = oracle.mdct_backward(np.eye(n // 2, dtype=np.float32))  # row k: the impulse at bin k
    err = np.abs(got - B.T).max(axis=1)
    k = int(err.argmax())
    print(f"\nn = {n}: worst impulse at bin {k}, max |error| = {err[k]:.3g}")
    assert err[k] <= 4 * IMDCT_MEASURED[n], (k, err[k])


# max |float32 round trip - float64 round trip| / peak of the signal, same measurement rule as IMDCT_MEASURED
TDAC_MEASURED = {128: 2.77e-07, 256: 1.45e-07, 512: 2.42e-07, 1024: 2.01e-07, 2048: 2.73e-07, 4096: 2.58e-07}


@pytest.mark.parametrize("n", IMDCT_SIZES)
def test_oracle_tdac_round_trip(oracle, n):
    """window, orc_mdct_forward, orc_mdct_backward, window and overlap-add of two consecutive blocks return the n/2
    samples the blocks share.  Against the same round trip in float64 (definition both ways, the same float32 window
    table), measured max |error| / signal peak:
    n = 128: 2.77e-07, 256: 1.45e-07, 512: 2.42e-07, 1024: 2.01e-07, 2048: 2.73e-07, 4096: 2.58e-07; bound 4 x that.  The
    float64 round trip itself returns the signal within 2e-7 x peak: each table entry is within 2^-24 of the window
    formula, so w[i]^2 + w[n/2-1-i]^2 is within 2 * 2^-24 * (w[i] + w[n/2-1-i]) <= 1.7e-7 of 1 (measured: 6.8e-8)."""
    from vorbis_aotuv_lancer_amd.tables import window_table
    h = n // 2
    rise = window_table(n)
    assert rise.dtype == np.float32 and rise.shape == (h,)
    w = np.concatenate([rise, rise[::-1]])
    x = np.random.default_rng(300 + n).standard_normal(n + h).astype(np.float32)
    blocks = np.stack([x[:n], x[h:]])
    B = imdct_basis(n)
    y64 = ((4.0 / n) * (blocks.astype(np.float64) * w) @ B) @ B.T * w
    want = y64[0, h:] + y64[1, :h]
    y32 = oracle.mdct_backward(oracle.mdct_forward(blocks * w)) * w
    got = y32[0, h:] + y32[1, :h]
    assert got.dtype == np.float32
    peak = float(np.abs(x[h:n]).max())
    assert np.abs(want - x[h:n]).max() <= 2e-7 * peak
    err = float(np.abs(got - want).max())
    print(f"\nn = {n}: round trip max |error| / peak = {err / peak:.3g}")
    assert err <= 4 * TDAC_MEASURED[n] * peak, (err / peak, TDAC_MEASURED[n])
