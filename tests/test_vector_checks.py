"""The checkers of oracle/vector_checks.py on CPU.  The componentwise GEMV bound accepts numpy's float64 GEMV (BLAS) at the
C3 headline size 4096 x 8192 and rejects a result with one product missing: one column, the 16-column tail of the padded
row, or one 128-row split of A^T.v.  The iteration envelope accepts the oracle against a third summation order of
itself and rejects a 1e-6 relative change of one component of d_x."""
import numpy as np
import pytest

from oracle import vector_checks as vc

M, N = 4096, 8192


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(11)
    A = rng.standard_normal((M, N))
    W = rng.standard_normal((2, N))
    V = rng.standard_normal((2, M))
    return A, W, V, vc.gemv_n_ref(A, W), vc.gemv_t_ref(A, V)


def test_bound_accepts_float64_blas(big):
    A, W, V, (yn, mn), (yt, mt) = big
    rn = vc.check_gemv(W @ A.T, yn, mn, N, "A.w")
    rt = vc.check_gemv(V @ A, yt, mt, M, "A^T.v")
    print(f"\n[measure] numpy float64 at {M}x{N}: A.w ratio {rn:.3g}, A^T.v ratio {rt:.3g}")
    assert rn <= 0.1 and rt <= 0.1
    # one row of the result alone, and an exact result
    assert vc.gemv_ratio(A[:7] @ W[0], *[x[:, :7] for x in vc.gemv_n_ref(A[:7], W[0])], N) <= 0.1
    assert vc.gemv_ratio(yn.astype(np.float64), yn, mn, N) <= 2 ** -10


def test_bound_rejects_one_missing_term(big):
    A, W, V, (yn, mn), (yt, mt) = big
    j = 5000
    no_col = W @ A.T - np.outer(W[:, j], A[:, j])                  # column j left out of every row sum
    assert vc.gemv_ratio(no_col, yn, mn, N) > 100
    with pytest.raises(AssertionError):
        vc.check_gemv(no_col, yn, mn, N)
    no_tail = W[:, :N - 16] @ A[:, :N - 16].T                      # the last 16 columns left out
    assert vc.gemv_ratio(no_tail, yn, mn, N) > 100
    keep = np.ones(M, dtype=bool)
    keep[1280:1408] = False                                        # row split 10 of A^T.v left out
    no_split = V[:, keep] @ A[keep]
    assert vc.gemv_ratio(no_split, yt, mt, M) > 100
    one = (V @ A).copy()
    one[1, 77] = yt[1, 77] + 2.0 * mt[1, 77] * 2 * M * vc.U        # twice the bound on one output of one vector
    assert 1.5 < vc.gemv_ratio(one, yt, mt, M) < 2.5


def test_zero_magnitude_outputs_must_be_exact():
    A = np.zeros((3, 40))
    A[0, 3] = 1.0
    w = np.ones(40)
    ref, mag = vc.gemv_n_ref(A, w)
    assert vc.gemv_ratio(A @ w, ref, mag, 40) == 0.0
    assert vc.gemv_ratio(A @ w + np.array([0.0, 1e-300, 0.0]), ref, mag, 40) == np.inf


def test_envelope_accepts_the_oracle_against_itself(built):
    from oracle import capi as oracle
    rng = np.random.default_rng(3)
    m, n = 150, 400
    A = rng.standard_normal((m, n)); b = rng.standard_normal(m); c = rng.standard_normal(n)
    x, z = np.exp(rng.uniform(-2, 2, n)), np.exp(rng.uniform(-2, 2, n))
    y = rng.standard_normal(m)
    ref, spread = vc.iteration_envelope(A, b, c, x, y, z, 0.7, 1.3, seed=1)
    assert any(spread[k] > 0 for k in vc.VEC_KEYS)
    assert max(vc.iteration_ratios(ref, ref, spread).values()) == 0.0
    # a third summation order of the oracle: the same LP, columns permuted by another P, un-permuted
    P = np.random.default_rng(2).permutation(n)
    inv = np.argsort(P)
    third = oracle.iteration(A[:, P], b, c[P], x[P], y, z[P], 0.7, 1.3)
    for k in ("x", "z", "d_x", "d_z"):
        third[k] = third[k][inv]
    third["info"] = 0
    r = vc.check_iteration(third, ref, spread)
    assert max(r.values()) <= 0.25, r
    # zero spread and a tight fixed bound: a 1e-6 relative change of one component of d_x fails
    bad = dict(third)
    bad["d_x"] = third["d_x"].copy()
    bad["d_x"][n - 1] *= 1.0 + 1e-6
    bad["d_x"][n - 1] += 1e-6 * np.abs(third["d_x"]).max()
    with pytest.raises(AssertionError):
        vc.check_iteration(bad, ref, spread, fixed=1e-9, K=1.0)
