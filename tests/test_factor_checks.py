"""The checkers of oracle/factor_checks.py on CPU: they accept LAPACK's factor (numpy.linalg.cholesky) and LAPACK's
solve with 4x margin to the bounds the GPU tests use (tests/test_gpu_factor_at_scale.py), and a single 1e-9-relative
change of one entry in an off-diagonal 128 x 128 tile of the factor fails those bounds, through the full residual and
through the probe vectors."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import factor_checks as fc

M_SIZE = 1100


@pytest.fixture(scope="module")
def wc():
    M, kappa = fc.well_conditioned(M_SIZE, 5)
    return M, kappa, np.linalg.cholesky(M)


def test_well_conditioned_family(wc):
    M, kappa, _ = wc
    w = np.linalg.eigvalsh(M)
    assert kappa <= 100 and w.min() > 0 and w.max() / w.min() <= kappa
    assert np.array_equal(M, M.T)
    # every 128 x 128 tile of the lower triangle is nonzero
    nb = (M_SIZE + 127) // 128
    assert all(np.abs(M[i * 128:(i + 1) * 128, j * 128:(j + 1) * 128]).min() > 0 for i in range(nb) for j in range(i + 1))


def test_checkers_accept_lapack(wc):
    M, kappa, L = wc
    X = fc.probe_columns(M_SIZE, np.random.default_rng(0))
    assert fc.factor_residual_c(L, M) <= fc.FACTOR_C / 4
    assert fc.probe_residual_c(L, M, X) <= fc.FACTOR_C / 4
    # the upper triangle of the factor is never read
    assert fc.factor_residual_c(L + np.triu(np.ones_like(L), 1), M) == fc.factor_residual_c(L, M)
    r = np.random.default_rng(1).standard_normal(M_SIZE)
    vt, cf = fc.refined_solution(M, r, cf=(L, True))
    v = sla.cho_solve(cf, r)
    assert fc.solve_residual(M, v, r) <= fc.SOLVE_RES_C * (M_SIZE + 1) * fc.U / 4
    assert fc.forward_error(v, vt) <= fc.SOLVE_FWD_C * kappa * (M_SIZE + 1) * fc.U / 4
    # the refined solution is a better one than LAPACK's
    Ml = M.astype(np.longdouble)
    assert np.abs(Ml @ vt - r).max() < np.abs(Ml @ v.astype(np.longdouble) - r).max()


@pytest.mark.parametrize("ti,tj", [(5, 2), (8, 0), (7, 6), (8, 4)])
def test_checkers_reject_one_wrong_tile_entry(wc, ti, tj):
    """The largest entry of off-diagonal tile (ti, tj) of the factor, changed by 1e-9 of itself."""
    M, _, L = wc
    blk = np.abs(L[ti * 128:(ti + 1) * 128, tj * 128:(tj + 1) * 128])
    i, j = np.unravel_index(blk.argmax(), blk.shape)
    Lp = L.copy()
    Lp[ti * 128 + i, tj * 128 + j] *= 1 + 1e-9
    assert fc.factor_residual_c(Lp, M) > fc.FACTOR_C
    assert fc.probe_residual_c(Lp, M, fc.probe_columns(M_SIZE, np.random.default_rng(0))) > fc.FACTOR_C


def test_probe_columns_cover_the_block_edges():
    X = fc.probe_columns(7000, np.random.default_rng(0), nrand=2)
    units = set(np.nonzero(X[:, 2:])[0])
    assert {0, 127, 128, 511, 512, 1023, 1024, 6143, 6144, 6999} <= units
    assert np.array_equal(np.abs(X[:, 2:]).sum(axis=0), np.ones(X.shape[1] - 2))


def test_adat_lower():
    rng = np.random.default_rng(2)
    A, d = rng.standard_normal((1500, 700)), np.exp(rng.uniform(-6, 6, 700))
    ref = (A * d) @ A.T
    got = fc.adat_lower(A, d)
    assert np.array_equal(got, np.tril(got))
    assert np.abs(got - np.tril(ref)).max() <= 1e-13 * np.abs(ref).max()
