"""The bounded form (lpipm_upload_bounded), without a device: the algebra the GPU path runs -- the bound block of
the explicit LP eliminated in closed form, so that the normal matrix stays m x m -- emulated in numpy inside the oracle's own
loop and compared with the unmodified oracle on the explicit form (the bound rows appended to the `ub` rows); the three exits;
the new symbols; the ValueError paths; ProblemBuilder without .upper.

The generator and the shape lists of tests/test_gpu_bounded.py live here, so that an input the oracle cannot solve fails in
this file."""
import functools

import numpy as np
import pytest

X_TOL = 1e-6


def planted_box(seed, m_ub, m_eq, nx, frac, tight):
    """A planted strictly complementary vertex of min c.x, A_ub x <= b_ub, A_eq x = b_eq, 0 <= x <= u with A_ub, A_eq ~ N(0,1):
    B = round(frac * nx) random columns with u_B ~ U(2.5, 4); k = n_active + m_eq basic columns with x* ~ U(1, 2) (strictly
    inside their bounds), n_active = min(max(max(nx // 2, m_eq) - m_eq, 0), m_ub) active `ub` rows; a share `tight` of the
    nonbasic bounded columns at x* = u with reduced cost -U(1, 2), the other nonbasic columns at 0 with reduced cost +U(1, 2);
    multipliers in [1, 2] on the active rows, free multipliers ~ N(0,1) on the `eq` rows.
    -> A_ub, b_ub, A_eq, b_eq, c, u (+inf: no bound), x*"""
    rng = np.random.default_rng(seed)
    A_ub = rng.standard_normal((m_ub, nx))
    A_eq = rng.standard_normal((m_eq, nx))
    nb = int(round(frac * nx))
    B = np.sort(rng.permutation(nx)[:nb])
    u = np.full(nx, np.inf)
    u[B] = rng.uniform(2.5, 4.0, nb)
    n_active = min(max(max(nx // 2, m_eq) - m_eq, 0), m_ub)
    k = n_active + m_eq
    order = rng.permutation(nx)
    basic, nonbasic = order[:k], order[k:]
    xs = np.zeros(nx)
    xs[basic] = rng.uniform(1, 2, k)
    rc = np.zeros(nx)
    rc[nonbasic] = rng.uniform(1, 2, nonbasic.shape[0])
    cand = nonbasic[np.isfinite(u[nonbasic])]
    at_u = cand[: int(round(tight * cand.shape[0]))]
    xs[at_u] = u[at_u]
    rc[at_u] = -rc[at_u]
    act = rng.permutation(m_ub)[:n_active]
    s = rng.uniform(1, 2, m_ub)
    s[act] = 0.0
    lam = np.zeros(m_ub)
    lam[act] = rng.uniform(1, 2, n_active)
    c = -A_ub.T @ lam + A_eq.T @ rng.standard_normal(m_eq) + rc
    return A_ub, A_ub @ xs + s, A_eq, A_eq @ xs, c, u, xs


# (seed, m_ub, m_eq, nx, frac, tight): m at 127, 129 and 257 (both sides of the 128-row padding), m + nb far beyond mp, the
# columns on both sides of the 256-column chunk, nb = 5 of 260 columns and nb = nx
SHAPES = [(1, 0, 2, 3, 1, .5), (2, 5, 0, 4, 1, 1), (3, 20, 4, 60, .5, .5), (4, 100, 27, 250, 1, .5), (5, 100, 29, 300, 1, .3),
          (6, 0, 130, 520, 1, .5), (7, 150, 50, 700, .3, 1), (8, 60, 3, 41, .9, .7), (9, 255, 2, 260, .02, 1)]
OPTION_SHAPE = SHAPES[3]
OPTIONS = [(), (("ip", False),), (("tol", 1e-6),)]
EXPLICIT_SHAPES = [SHAPES[2], SHAPES[3], SHAPES[7], SHAPES[8]]         # the bounded upload against ctx.upload of the explicit problem


def ids(shapes):
    return [f"s{s}-{mu}+{me}x{nx}-f{fr}-t{t}" for s, mu, me, nx, fr, t in shapes]


def exits():
    """name -> (A_ub, b_ub, A_eq, b_eq, c, u, expected status): infeasible by its bounds; unbounded along a column without a
    bound; bounded only by its bounds (x = (3, 2))."""
    z3, z2 = np.zeros((0, 3)), np.zeros((0, 2))
    return {
        "infeasible": (z3, np.zeros(0), np.ones((1, 3)), np.array([10.0]), np.ones(3), np.ones(3), 5),
        "unbounded": (z3, np.zeros(0), np.array([[1.0, 1.0, 0.0]]), np.array([1.0]), np.array([0.0, 0.0, -1.0]),
                      np.array([1.0, np.inf, np.inf]), 6),
        "by_bounds": (np.array([[1.0, -1.0]]), np.array([1.0]), z2, np.zeros(0), np.array([-1.0, -1.0]), np.array([3.0, 2.0]), 0),
    }


def bounded_columns(u):
    return np.flatnonzero(np.isfinite(u))


def explicit_parts(A_ub, b_ub, u):
    """The explicit form's `ub` block: the bound rows x_j <= u_j appended to the `ub` rows -> A_ub', b_ub'."""
    B = bounded_columns(u)
    E = np.zeros((B.shape[0], A_ub.shape[1]))
    E[np.arange(B.shape[0]), B] = 1.0
    return np.vstack([A_ub, E]), np.concatenate([b_ub, u[B]])


def explicit_slack_form(A_ub, b_ub, A_eq, b_eq, c, u):
    """The slack form of the explicit LP as lpipm_upload_ub_eq assembles it: rows [ub; bounds; eq], columns [x; ub slacks; w]."""
    Au, bu = explicit_parts(A_ub, b_ub, u)
    mu, me = Au.shape[0], A_eq.shape[0]
    A = np.block([[Au, np.eye(mu)], [A_eq, np.zeros((me, mu))]])
    return A, np.concatenate([bu, b_eq]), np.concatenate([c, np.zeros(mu)])


def ext_form(A_ub, b_ub, A_eq, b_eq, c, u):
    """A_ext = [[A, 0], [E_B, I]] of the bounded upload, A the slack form without the bounds: rows [ub; eq; bounds], the same
    columns as the explicit form.  -> A_ext, b_ext, c_ext"""
    B = bounded_columns(u)
    m_ub, m_eq, nx, nb = A_ub.shape[0], A_eq.shape[0], c.shape[0], B.shape[0]
    A = np.block([[A_ub, np.eye(m_ub)], [A_eq, np.zeros((m_eq, m_ub))]])
    E = np.zeros((nb, nx + m_ub))
    E[np.arange(nb), B] = 1.0
    Ax = np.block([[A, np.zeros((m_ub + m_eq, nb))], [E, np.eye(nb)]])
    return Ax, np.concatenate([b_ub, b_eq, u[B]]), np.concatenate([c, np.zeros(m_ub + nb)])


def make_box_solver(n, m, B):
    """oracle_np._EqSolver with sym_solve replaced by the algebra of lpipm_upload_bounded on A_ext = [[A, 0], [E_B, I]], A m x n."""
    import scipy.linalg as sla
    from oracle import oracle_np
    B = np.asarray(B)

    class BoxSolver(oracle_np._EqSolver):
        def __init__(self, A_ext, x, z, solver_type, timing):
            self.timing, self.kind = timing, 0
            self.A = A_ext[:m, :n]
            self.dx, self.dw = x[:n] / z[:n], x[n:] / z[n:]
            self.s = self.dx[B] + self.dw
            self.Dt = self.dx.copy()
            self.Dt[B] = 1.0 / (z[:n][B] / x[:n][B] + z[n:] / x[n:])
            try:
                self.L = np.linalg.cholesky(self.A @ (self.Dt[:, None] * self.A.T))
                self.ok = True
            except np.linalg.LinAlgError:
                self.ok = False

        def sym_solve(self, A_ext, r1, r2):
            r1x, r1w, r21, r22 = r1[:n], r1[n:], r2[:m], r2[m:]
            rx, rw = self.dx[B] / self.s, self.dw / self.s
            W = self.Dt * r1x
            W[B] = self.Dt[B] * (r1x[B] - r1w) - rx * r22
            r = r21 + self.A @ W
            v1 = sla.solve_triangular(self.L, sla.solve_triangular(self.L, r, lower=True, check_finite=False), lower=True,
                                      trans=1, check_finite=False)
            t = self.A.T @ v1
            ux = self.Dt * (t - r1x)
            g = self.Dt[B] * (t[B] - r1x[B] + r1w)
            ux[B] = g + rx * r22
            uw = -g + rw * r22
            v2 = r1w + uw / self.dw
            return np.concatenate([ux, uw]), np.concatenate([v1, v2])

    return BoxSolver


def solve_np(A, b, c, kw=(), solver=None):
    from oracle import oracle_np
    keep = oracle_np._EqSolver
    try:
        if solver is not None:
            oracle_np._EqSolver = solver
        return oracle_np.solve(A, b, c, opts=oracle_np.Opts(**dict(kw)))
    finally:
        oracle_np._EqSolver = keep


@functools.lru_cache(maxsize=None)
def oracle_explicit(case, kw=()):
    """The unmodified numpy oracle on the explicit form of a shape (computed once, shared)."""
    return solve_np(*explicit_slack_form(*planted_box(*case)[:6]), kw)


def emulated(lp, kw=()):
    A_ub, b_ub, A_eq, b_eq, c, u = lp
    n, m = c.shape[0] + A_ub.shape[0], A_ub.shape[0] + A_eq.shape[0]
    return solve_np(*ext_form(*lp), kw, solver=make_box_solver(n, m, bounded_columns(u)))


@pytest.mark.parametrize("case", SHAPES, ids=ids(SHAPES))
def test_emulated_algebra_matches_the_oracle_on_the_explicit_form(case):
    lp = planted_box(*case)
    ref = oracle_explicit(case)
    got = emulated(lp[:6])
    assert ref.status == 0 and got.status == 0, (ref.status, got.status)
    assert got.iterations == ref.iterations, (got.iterations, ref.iterations)
    err = np.abs(got.x_slack - ref.x_slack).max()
    nx = case[3]
    planted = np.abs(ref.x_slack[:nx] - lp[6]).max()
    print(f"\n[measure] {case}: {got.iterations} iterations, max|x - x_explicit| {err:.3g}, oracle to the planted vertex {planted:.3g}")
    assert err <= X_TOL, err
    assert abs(got.fun - ref.fun) <= 1e-6 * max(1.0, abs(ref.fun))


@pytest.mark.parametrize("kw", OPTIONS[1:], ids=["ip0", "tol1e-6"])
def test_emulated_algebra_under_options(kw):
    lp = planted_box(*OPTION_SHAPE)
    ref = oracle_explicit(OPTION_SHAPE, kw)
    got = emulated(lp[:6], kw)
    assert got.status == ref.status == 0
    assert got.iterations == ref.iterations
    assert np.abs(got.x_slack - ref.x_slack).max() <= X_TOL


@pytest.mark.parametrize("name", ["infeasible", "unbounded", "by_bounds"])
def test_the_three_exits_behave_alike(name):
    *lp, status = exits()[name]
    ref = solve_np(*explicit_slack_form(*lp))
    got = emulated(tuple(lp))
    print(f"\n[measure] {name}: status {got.status} / {ref.status}, {got.iterations} / {ref.iterations} iterations")
    assert got.status == ref.status == status
    assert got.iterations == ref.iterations
    if status == 0:
        assert np.abs(got.x_slack - ref.x_slack).max() <= X_TOL
        assert np.abs(got.x_slack[:2] - np.array([3.0, 2.0])).max() <= X_TOL


def test_symbols_and_prototypes(built):
    import ctypes as C
    from lp_amd import _capi
    lib = _capi.lib()
    for name in ("lpipm_upload_bounded", "lpipm_k_bounded_normal", "lpipm_k_bounded_sym_solve"):
        assert getattr(lib, name).restype is C.c_int
    assert len(lib.lpipm_upload_bounded.argtypes) == len(lib.lpipm_upload_ub_eq.argtypes) + 1 == 13
    assert len(lib.lpipm_k_bounded_normal.argtypes) == 3
    assert len(lib.lpipm_k_bounded_sym_solve.argtypes) == len(lib.lpipm_k_tall_sym_solve.argtypes) == 8
    # without a context nothing is touched: a shape without rows is Unconstrained first, a null context a bad argument
    c = np.ones(3)
    u = np.array([1.0, np.inf, 2.0])
    cp, up = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (c, u))
    assert lib.lpipm_upload_bounded(None, 3, 0, None, 3, None, 0, None, 3, None, cp, 0.0, up) == _capi.UNCONSTRAINED
    assert lib.lpipm_upload_bounded(None, 3, 0, None, 3, None, 0, None, 3, None, cp, 0.0, None) == _capi.UNCONSTRAINED
    assert lib.lpipm_upload_bounded(None, 3, 0, None, 3, None, 1, cp, 3, cp, cp, 0.0, up) == _capi.ERR_BAD_ARGUMENT
    assert lib.lpipm_k_bounded_normal(None, cp, cp) == _capi.ERR_BAD_ARGUMENT


def test_value_errors():
    import lp_amd
    cx = lp_amd.Context.__new__(lp_amd.Context)          # no device: the checks come before the library is called
    c = np.ones(3)
    ub = lp_amd.Problem.target(c).ub(np.ones((2, 3)), np.ones(2))
    with pytest.raises(ValueError):
        lp_amd.Context.upload(cx, ub.upper([1.0, np.inf, 2.0]).build(), tall=True)
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        lp_amd.Problem.target(c).ub(np.ones((2, 3)), np.ones(2)).upper([1.0, 2.0]).build()
    for bad in (np.nan, -np.inf):
        with pytest.raises(lp_amd.InvalidParameter):
            lp_amd.Problem.target(c).ub(np.ones((2, 3)), np.ones(2)).upper([1.0, bad, 2.0]).build()


def test_builder_without_upper_builds_what_it_built_before():
    import lp_amd
    A_ub, b_ub, A_eq, b_eq, c, u, _ = planted_box(*SHAPES[2])
    plain = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build()
    assert plain.upper() is None and plain.n_bounded() == 0
    assert plain.n_slack() == A_ub.shape[0] and plain.dtype == np.float64
    assert plain.A().shape == (A_ub.shape[0] + A_eq.shape[0], c.shape[0] + A_ub.shape[0])
    x = np.arange(float(plain.A().shape[1]))
    assert np.array_equal(plain.denormalize_x_into(x), x[: c.shape[0]])
    y = np.arange(float(plain.A().shape[0]))
    y_ub, y_eq, red = plain.denormalize_duals(y, x)
    assert np.array_equal(y_ub, y[: A_ub.shape[0]]) and np.array_equal(y_eq, y[A_ub.shape[0]:]) and np.array_equal(red, x[: c.shape[0]])
    boxed = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).upper(u).build()
    nb = int(np.isfinite(u).sum())
    assert boxed.n_bounded() == nb and np.array_equal(boxed.upper(), u)
    assert np.array_equal(boxed.A(), plain.A()) and np.array_equal(boxed.b(), plain.b()) and np.array_equal(boxed.c(), plain.c())
    xe = np.arange(float(plain.A().shape[1] + nb))
    assert np.array_equal(boxed.denormalize_x_into(xe), xe[: c.shape[0]])
    v = boxed.denormalize_bound_duals(xe)
    assert np.array_equal(v[np.isfinite(u)], xe[xe.shape[0] - nb:]) and not v[~np.isfinite(u)].any()
    f32 = lp_amd.Problem.target(c.astype(np.float32)).ub(A_ub.astype(np.float32), b_ub.astype(np.float32)).build()
    assert f32.dtype == np.float32 and f32.upper() is None
