"""The tall form with equality rows (lpipm_upload_ub_eq_tall), without a device: the algebra the GPU path runs
-- K on the `ub` rows, a Schur complement on K's factor for the `eq` rows, the solve on K split into its forward and backward
halves -- emulated in numpy inside the oracle's own loop and compared with the unmodified oracle; the condition every parity
shape of tests/test_gpu_tall_eq.py must meet; the new symbols; the ValueError paths of Context.upload_tall_eq.

The generator and the shapes of the GPU tests live here, so that an input the oracle itself cannot solve fails in this file."""
import functools

import numpy as np
import pytest

X_TOL = 1e-6


def planted_eq(seed, m, nx, me):
    """A planted nondegenerate, strictly complementary vertex of min c^T x, X x <= b, A_eq x = b_eq, x >= 0 with X, A_eq ~ N(0,1):
    k = max(nx // 2, me) basic structural variables, k - me active `ub` rows (k + the m - (k - me) positive slacks = m + me basic
    variables), multipliers in [1, 2] on the active rows and on the nonbasic columns, free multipliers ~ N(0,1) on the `eq` rows.
    -> X, b, A_eq, b_eq, c, x*"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    Ae = rng.standard_normal((me, nx))
    k = min(nx, max(nx // 2, me))
    na = max(k - me, 0)
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:na]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, na)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    c = -X.T @ lam + Ae.T @ rng.standard_normal(me) + mu
    return X, b, Ae, Ae @ xs, c, xs


def planted_face(seed, m, nx, me):
    """A planted strictly complementary optimum that is NOT a vertex: about 60 % of the columns positive, a random set of active
    `ub` rows (many more of them than positive columns when m >> nx), so the optimal x need not be unique and only the optimal
    value f* = c^T x* is pinned.  On such LPs with m >> nx the m x m normal matrix of the last iterations is numerically singular.
    A second generator because planted_eq does not give such an input: its 4096x32+8 at seed 1 is a vertex with 8 active rows, and
    the unmodified oracle solves it (Ok in 7 iterations), so it cannot stand for "a shape where the oracle itself fails".
    -> X, b, A_eq, b_eq, c, x*"""
    r = np.random.default_rng(seed)
    X = r.standard_normal((m, nx)); Ae = r.standard_normal((me, nx))
    xs = np.where(r.random(nx) < 0.6, r.uniform(1, 2, nx), 0.0)
    act = r.random(m) < min(0.5, (nx - me) / (2.0 * m) + 0.05)
    s = np.where(act, 0.0, r.uniform(1, 2, m))
    b = X @ xs + s
    yu = np.where(act, -r.uniform(1, 2, m), 0.0); ye = r.standard_normal(me)
    zx = np.where(xs > 0, 0.0, r.uniform(1, 2, nx))
    return X, b, Ae, Ae @ xs, X.T @ yu + Ae.T @ ye + zx, xs


FACE_CASE = (1, 4096, 32, 8)         # the oracle's own m x m Cholesky fails here in its last iteration; the reduced form does not


def slack_form(X, b, Ae, be, c):
    m, me = X.shape[0], Ae.shape[0]
    A = np.block([[X, np.eye(m)], [Ae, np.zeros((me, m))]])
    return A, np.concatenate([b, be]), np.concatenate([c, np.zeros(m)])


def permuted(X, Ae, c, seed):
    """The same LP with its structural columns permuted: -> X', A_eq', c', perm (x' = x[perm])."""
    perm = np.random.default_rng(7000 + seed).permutation(X.shape[1])
    return X[:, perm], Ae[:, perm], c[perm], perm


# (seed, m_ub, nx, m_eq): the parity cases.  HOST: emulated below; GPU: whole solves of tests/test_gpu_tall_eq.py
HOST_SHAPES = [(1, 3, 2, 1), (1, 40, 8, 2), (1, 300, 40, 5), (1, 300, 40, 39), (1, 1100, 130, 17)]
GPU_SHAPES = [(1, 300, 40, 1), (1, 300, 40, 5), (1, 300, 40, 39), (1, 1100, 130, 17), (1, 1300, 600, 130)]
OPTION_SHAPE = (1, 300, 40, 5)
OPTIONS = [(), (("ip", False),), (("tol", 1e-6),), (("max_iter", 3),)]


def _ids(shapes):
    return [f"{m}x{nx}+{me}" for _, m, nx, me in shapes]


def make_tall_eq_solver(nx, m_ub):
    """oracle_np._EqSolver with sym_solve replaced by the algebra of lpipm_upload_ub_eq_tall on A = [[X I], [A_eq 0]]."""
    import scipy.linalg as sla
    from oracle import oracle_np

    class TallEqSolver(oracle_np._EqSolver):
        def __init__(self, A, x, z, solver_type, timing):
            self.timing, self.kind = timing, 0
            self.Dinv = x / z
            X, Ae = A[:m_ub, :nx], A[m_ub:, :nx]
            self.X, self.Ae = X, Ae
            self.Ws = z[nx:] / x[nx:]
            K = X.T @ (self.Ws[:, None] * X) + np.diag(z[:nx] / x[:nx])
            try:
                self.L = np.linalg.cholesky(K)
                self.Zt = sla.solve_triangular(self.L, Ae.T, lower=True, check_finite=False).T      # Zt = A_eq.L^-T
                self.LS = np.linalg.cholesky(self.Zt @ self.Zt.T)
                self.ok = True
            except np.linalg.LinAlgError:
                self.ok = False

        def sym_solve(self, A, r1, r2):
            tri = lambda L, r, trans: sla.solve_triangular(L, r, lower=True, trans=trans, check_finite=False)
            r1x, r1s, r2u, r2e = r1[:nx], r1[nx:], r2[:m_ub], r2[m_ub:]
            t = self.Ws * r2u + r1s
            g = self.X.T @ t - r1x
            w = tri(self.L, g, 0)                                    # forward half only
            h = r2e - self.Zt @ w
            ve = tri(self.LS, tri(self.LS, h, 0), 1)
            w = w + self.Zt.T @ ve
            ux = tri(self.L, w, 1)                                   # backward half only
            us = r2u - self.X @ ux
            vu = self.Ws * us + r1s
            return np.concatenate([ux, us]), np.concatenate([vu, ve])

    return TallEqSolver


def _solve_np(A, b, c, kw=(), solver=None):
    from oracle import oracle_np
    keep = oracle_np._EqSolver
    try:
        if solver is not None:
            oracle_np._EqSolver = solver
        return oracle_np.solve(A, b, c, opts=oracle_np.Opts(**dict(kw)))
    finally:
        oracle_np._EqSolver = keep


@functools.lru_cache(maxsize=None)
def oracle_pair(case, kw=()):
    """The unmodified numpy oracle on the case as generated and with its structural columns permuted (x mapped back)."""
    seed, m, nx, me = case
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    ref = _solve_np(*slack_form(X, b, Ae, be, c), kw)
    Xp, Aep, cp, perm = permuted(X, Ae, c, seed)
    alt = _solve_np(*slack_form(Xp, b, Aep, be, cp), kw)
    if alt.x_slack is not None:
        back = alt.x_slack.copy()
        back[perm] = alt.x_slack[:nx]
        alt.x_slack = back
    return ref, alt


@pytest.mark.parametrize("case", sorted(set(HOST_SHAPES + GPU_SHAPES)), ids=_ids(sorted(set(HOST_SHAPES + GPU_SHAPES))))
def test_parity_shapes_are_ones_the_oracle_solves(case):
    """A condition on the inputs, not a measurement: Ok as generated and with permuted columns, and the two runs agree."""
    ref, alt = oracle_pair(case)
    assert ref.status == 0 and alt.status == 0, (ref.status, alt.status)
    spread = np.abs(ref.x_slack - alt.x_slack).max()
    print(f"\n[measure] {case}: {ref.iterations} / {alt.iterations} iterations, oracle spread under a column permutation {spread:.3g}")
    assert spread <= X_TOL, spread
    xs = planted_eq(*case)[5]
    assert np.abs(ref.x_slack[:case[2]] - xs).max() <= X_TOL


@pytest.mark.parametrize("case", HOST_SHAPES, ids=_ids(HOST_SHAPES))
def test_emulated_algebra_matches_the_oracle(case):
    seed, m, nx, me = case
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    ref, _ = oracle_pair(case)
    got = _solve_np(*slack_form(X, b, Ae, be, c), solver=make_tall_eq_solver(nx, m))
    assert got.status == ref.status == 0
    assert got.iterations == ref.iterations, (got.iterations, ref.iterations)
    err = np.abs(got.x_slack - ref.x_slack).max()
    print(f"\n[measure] emulation {m}x{nx}+{me}: {got.iterations} iterations, max|dx| {err:.3g}")
    assert err <= X_TOL, err


@pytest.mark.parametrize("kw", OPTIONS[1:], ids=["ip0", "tol1e-6", "max_iter3"])
def test_emulated_algebra_under_options(kw):
    seed, m, nx, me = OPTION_SHAPE
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    ref, _ = oracle_pair(OPTION_SHAPE, kw)
    got = _solve_np(*slack_form(X, b, Ae, be, c), kw, solver=make_tall_eq_solver(nx, m))
    assert got.status == ref.status == (7 if dict(kw).get("max_iter") == 3 else 0)
    assert got.iterations == ref.iterations
    assert np.abs(got.x_slack - ref.x_slack).max() <= X_TOL


def test_emulated_algebra_reaches_the_optimum_where_the_oracle_fails():
    """4096x32+8 on planted_face: not a parity case -- the unmodified oracle ends in NumericalProblem (its m x m pivot), the
    reduced form in Ok at the planted optimal value.  The bounds of the GPU test."""
    seed, m, nx, me = FACE_CASE
    X, b, Ae, be, c, xs = planted_face(seed, m, nx, me)
    A, bb, cc = slack_form(X, b, Ae, be, c)
    assert _solve_np(A, bb, cc).status == 2
    got = _solve_np(A, bb, cc, solver=make_tall_eq_solver(nx, m))
    x, fstar = got.x_slack, float(c @ xs)
    assert got.status == 0
    assert abs(got.fun - fstar) <= 1e-6 * max(1.0, abs(fstar))
    assert max(np.maximum(X @ x[:nx] - b, 0.0).max(), np.abs(Ae @ x[:nx] - be).max(), np.maximum(-x, 0.0).max()) <= 1e-6


def test_symbols_and_prototypes(built):
    import ctypes as C
    from lp_amd import _capi
    lib = _capi.lib()
    for name in ("lpipm_upload_ub_eq_tall", "lpipm_k_tall_schur"):
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
    assert len(lib.lpipm_upload_ub_eq_tall.argtypes) == len(lib.lpipm_upload_ub_eq.argtypes) == 12
    assert len(lib.lpipm_k_tall_schur.argtypes) == 3
    # without a context nothing is touched: the null context is a bad argument, a shape without rows Unconstrained first
    c = np.ones(3)
    cp = c.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.lpipm_upload_ub_eq_tall(None, 3, 0, None, 3, None, 0, None, 3, None, cp, 0.0) == _capi.UNCONSTRAINED
    assert lib.lpipm_k_tall_schur(None, cp, cp) == _capi.ERR_BAD_ARGUMENT


def test_upload_tall_eq_value_errors():
    import lp_amd
    cx = lp_amd.Context.__new__(lp_amd.Context)          # no device: the checks come before the library is called
    c = np.ones(3)
    with pytest.raises(ValueError):
        lp_amd.Context.upload_tall_eq(cx, lp_amd.Problem.target(c).eq(np.ones((1, 3)), np.ones(1)).build())
    with pytest.raises(ValueError):
        lp_amd.Context.upload(cx, lp_amd.Problem.target(c).ub(np.ones((2, 3)), np.ones(2)).eq(np.ones((1, 3)), np.ones(1)).build(),
                              tall=True)
