"""General column bounds (lpipm_upload_bounds), without a device: the algebra the GPU path runs -- shifts and
reflections into the primed LP, the bound block AND the free block of the extended LP eliminated in closed form, so that the
normal matrix stays m x m and a free column stays one column -- emulated in numpy inside the oracle's own loop and compared
with the unmodified oracle on the explicit form of the primed LP (free columns duplicated and negated, bound rows appended);
the exits; the new symbol; the refusals that need no device; the builder's error paths; ProblemBuilder without .lower.

The two halves of a free column are determined only up to a common shift (the split has the ray (1, 1)): every comparison
is on the NET value x+ - x-, never on the halves.

The generator, the transforms and the shape lists of tests/test_gpu_bounds.py live here, so that an input the oracle cannot
solve fails in this file."""
import functools

import numpy as np
import pytest

from test_bounded_host import X_TOL, solve_np

OPTIONS = [(), (("ip", False),), (("tol", 1e-6),)]


def planted_bounds(seed, m_ub, m_eq, nx, frac_bounded, frac_free, tight):
    """planted_box's planted strictly complementary vertex, in the primed variables x' >= 0, with nf = round(frac_free * nx)
    free columns disjoint from the nb = round(frac_bounded * nx) bounded ones: free columns are always basic, x'* ~ +-U(1, 2),
    reduced cost 0; n_active = min(max(max(nx // 2, m_eq + nf) - m_eq, 0), m_ub) active `ub` rows, so that the basis can hold
    them.  On top of it the caller's LP x = t + sigma x': shifts t_j ~ U(-3, 3) on about 70 % of the non-free columns, a
    reflection on a third of the columns that have neither an upper bound nor freedom.
    -> the caller's A_ub, b_ub, A_eq, b_eq, c, lower, upper, and the caller's x*"""
    rng = np.random.default_rng(seed)
    A_ub = rng.standard_normal((m_ub, nx))
    A_eq = rng.standard_normal((m_eq, nx))
    nb, nf = int(round(frac_bounded * nx)), int(round(frac_free * nx))
    assert nb + nf <= nx
    cols = rng.permutation(nx)
    B, F = np.sort(cols[:nb]), np.sort(cols[nb: nb + nf])
    u = np.full(nx, np.inf)
    u[B] = rng.uniform(2.5, 4.0, nb)
    free = np.zeros(nx, dtype=bool)
    free[F] = True
    n_active = min(max(max(nx // 2, m_eq + nf) - m_eq, 0), m_ub)
    assert n_active + m_eq >= nf, (n_active, m_eq, nf)
    k = n_active + m_eq
    assert k <= nx
    rest = rng.permutation(np.flatnonzero(~free))
    basic, nonbasic = np.concatenate([F, rest[: k - nf]]), rest[k - nf:]
    xs = np.zeros(nx)
    xs[basic] = rng.uniform(1, 2, basic.shape[0])
    xs[F] *= rng.choice([-1.0, 1.0], nf)
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
    cp = -A_ub.T @ lam + A_eq.T @ rng.standard_normal(m_eq) + rc
    bp_ub, bp_eq = A_ub @ xs + s, A_eq @ xs
    # the caller's LP
    t = np.where(rng.uniform(size=nx) < 0.7, rng.uniform(-3, 3, nx), 0.0)
    t[F] = 0.0
    plain = np.flatnonzero(~free & ~np.isfinite(u))
    sigma = np.ones(nx)
    sigma[plain[rng.uniform(size=plain.shape[0]) < 1.0 / 3.0]] = -1.0
    lower, upper = t.copy(), t + u
    refl = sigma < 0
    lower[refl], upper[refl] = -np.inf, t[refl]
    lower[F] = -np.inf
    Au, Ae = A_ub * sigma, A_eq * sigma                     # A = A'.diag(sigma)
    return Au, bp_ub + Au @ t, Ae, bp_eq + Ae @ t, sigma * cp, lower, upper, t + sigma * xs


def shape_with_one_free(seed, m_ub, m_eq, nx, where):
    """A planted LP whose only free column is column `where` (0 or nx - 1): planted_bounds with a third of the columns bounded,
    its columns renumbered so that the free one lands there."""
    A_ub, b_ub, A_eq, b_eq, c, lower, upper, xs = planted_bounds(seed, m_ub, m_eq, nx, 1.0 / 3.0, 1.0 / nx, .5)
    f = int(np.flatnonzero(np.isinf(lower) & np.isinf(upper))[0])
    perm = np.arange(nx)
    perm[[f, where]] = perm[[where, f]]
    return A_ub[:, perm], b_ub, A_eq[:, perm], b_eq, c[perm], lower[perm], upper[perm], xs[perm]


# (seed, m_ub, m_eq, nx, frac_bounded, frac_free, tight): m at 127, 129 and 257 (both sides of the 128-row padding), n across
# the 256-column chunk, na = 515, free columns only, and one free column at either end of the structural block
SHAPES = [(1, 0, 3, 4, .25, .5, .5), (2, 5, 0, 4, .5, .25, 1), (3, 20, 4, 60, .4, .2, .5), (4, 100, 27, 250, .5, .3, .5),
          (5, 100, 29, 300, .6, .4, .3), (6, 0, 130, 520, .5, .2, .5), (7, 150, 50, 700, .3, .1, 1), (8, 60, 3, 41, .5, .4, .7),
          (9, 255, 2, 260, .02, .5, 1), (11, 30, 0, 64, 0, .3, 0), ("last", 12, 20, 5, 40), ("first", 13, 20, 5, 40)]
OPTION_SHAPE = SHAPES[3]
EXPLICIT_SHAPES = [SHAPES[2], SHAPES[3], SHAPES[7], SHAPES[8]]


def ids(shapes):
    return ["-".join(str(v) for v in s) for s in shapes]


@functools.lru_cache(maxsize=None)
def lp_of(case):
    if case[0] == "last":
        return shape_with_one_free(*case[1:], case[4] - 1)
    if case[0] == "first":
        return shape_with_one_free(*case[1:], 0)
    return planted_bounds(*case)


def classes(lower, upper):
    """-> sigma, t, u' (+inf: no bound row), B, F of the issue's table."""
    has_l, has_u = np.isfinite(lower), np.isfinite(upper)
    sigma = np.where(~has_l & has_u, -1.0, 1.0)
    t = np.where(has_l, lower, np.where(has_u, upper, 0.0))
    up = np.where(has_l & has_u, upper - lower, np.inf)
    return sigma, t, up, np.flatnonzero(has_l & has_u), np.flatnonzero(~has_l & ~has_u)


def primed(lp):
    """The primed LP of the caller's (A_ub, b_ub, A_eq, b_eq, c, lower, upper): A' = A.diag(sigma), b' = b - A.t, c' = sigma c,
    c0' = c.t -> (A_ub', b_ub', A_eq', b_eq', c', u', F, sigma, t, c0')"""
    A_ub, b_ub, A_eq, b_eq, c, lower, upper = lp
    sigma, t, up, _, F = classes(lower, upper)
    return A_ub * sigma, b_ub - A_ub @ t, A_eq * sigma, b_eq - A_eq @ t, sigma * c, up, F, sigma, t, float(c @ t)


def explicit_parts(lp):
    """The explicit form of the primed LP as `ub` / `eq` blocks: columns [x'; x^-_F], the bound rows appended to the `ub` rows.
    -> A_ub, b_ub, A_eq, b_eq, c"""
    Au, bu, Ae, be, cp, up, F, *_ = primed(lp)
    B = np.flatnonzero(np.isfinite(up))
    nx, nf = cp.shape[0], F.shape[0]
    E = np.zeros((B.shape[0], nx + nf))
    E[np.arange(B.shape[0]), B] = 1.0
    return (np.vstack([np.hstack([Au, -Au[:, F]]), E]), np.concatenate([bu, up[B]]), np.hstack([Ae, -Ae[:, F]]), be,
            np.concatenate([cp, -cp[F]]))


def explicit_slack_form(lp):
    """The slack form lpipm_upload_ub_eq assembles of explicit_parts: rows [ub; bounds; eq], columns [x'; x^-; ub slacks; w]."""
    Au, bu, Ae, be, c = explicit_parts(lp)
    mu, me = Au.shape[0], Ae.shape[0]
    return np.block([[Au, np.eye(mu)], [Ae, np.zeros((me, mu))]]), np.concatenate([bu, be]), np.concatenate([c, np.zeros(mu)])


def ext_form(lp):
    """A_ext = [[A', 0, -A'_F], [E_B, I, 0]] of the upload, A' the slack form of the primed LP: rows [ub; eq; bounds], columns
    [x'; ub slacks; w; x^-].  -> A_ext, b_ext, c_ext"""
    Au, bu, Ae, be, cp, up, F, *_ = primed(lp)
    B = np.flatnonzero(np.isfinite(up))
    m_ub, m_eq, nx, nb, nf = Au.shape[0], Ae.shape[0], cp.shape[0], B.shape[0], F.shape[0]
    A = np.block([[Au, np.eye(m_ub)], [Ae, np.zeros((m_eq, m_ub))]])
    E = np.zeros((nb, nx + m_ub))
    E[np.arange(nb), B] = 1.0
    Ax = np.block([[A, np.zeros((m_ub + m_eq, nb)), -A[:, F]], [E, np.eye(nb), np.zeros((nb, nf))]])
    return Ax, np.concatenate([bu, be, up[B]]), np.concatenate([cp, np.zeros(m_ub + nb), -cp[F]])


def caller_x(lp, x_net):
    """The caller's structural values of the primed net values."""
    sigma, t, *_ = classes(lp[5], lp[6])
    return t + sigma * x_net


def net_of_explicit(lp, x_slack):
    nx = lp[4].shape[0]
    F = classes(lp[5], lp[6])[4]
    net = np.array(x_slack[:nx])
    net[F] -= x_slack[nx: nx + F.shape[0]]
    return net


def net_of_ext(lp, x_ext):
    nx = lp[4].shape[0]
    F = classes(lp[5], lp[6])[4]
    net = np.array(x_ext[:nx])
    if F.shape[0]:
        net[F] -= x_ext[x_ext.shape[0] - F.shape[0]:]
    return net


def make_bounds_solver(n, m, B, F):
    """oracle_np._EqSolver with sym_solve replaced by the algebra of lpipm_upload_bounds on A_ext, A' m x n: the lines of the
    bounded form outside F, and on F  D~ = dx + dm,  W = dx r1_x - dm r1_m,  u_x = dx (t - r1_x),  u_m = dm (-t - r1_m)."""
    import scipy.linalg as sla
    from oracle import oracle_np
    B, F = np.asarray(B), np.asarray(F)
    nb = B.shape[0]

    class BoundsSolver(oracle_np._EqSolver):
        def __init__(self, A_ext, x, z, solver_type, timing):
            self.timing, self.kind = timing, 0
            self.A = A_ext[:m, :n]
            d = x / z
            self.dx, self.dw, self.dm = d[:n], d[n: n + nb], d[n + nb:]
            self.s = self.dx[B] + self.dw
            self.Dt = self.dx.copy()
            self.Dt[B] = 1.0 / (z[:n][B] / x[:n][B] + z[n: n + nb] / x[n: n + nb])
            self.Dt[F] = self.dx[F] + self.dm
            try:
                self.L = np.linalg.cholesky(self.A @ (self.Dt[:, None] * self.A.T))
                self.ok = True
            except np.linalg.LinAlgError:
                self.ok = False

        def sym_solve(self, A_ext, r1, r2):
            r1x, r1w, r1m, r21, r22 = r1[:n], r1[n: n + nb], r1[n + nb:], r2[:m], r2[m:]
            rx, rw = self.dx[B] / self.s, self.dw / self.s
            W = self.Dt * r1x
            W[B] = self.Dt[B] * (r1x[B] - r1w) - rx * r22
            W[F] = self.dx[F] * r1x[F] - self.dm * r1m
            r = r21 + self.A @ W
            v1 = sla.solve_triangular(self.L, sla.solve_triangular(self.L, r, lower=True, check_finite=False), lower=True,
                                      trans=1, check_finite=False)
            t = self.A.T @ v1
            ux = self.Dt * (t - r1x)
            g = self.Dt[B] * (t[B] - r1x[B] + r1w)
            ux[B] = g + rx * r22
            uw = -g + rw * r22
            ux[F] = self.dx[F] * (t[F] - r1x[F])
            um = self.dm * (-t[F] - r1m)
            v2 = r1w + uw / self.dw
            return np.concatenate([ux, uw, um]), np.concatenate([v1, v2])

    return BoundsSolver


@functools.lru_cache(maxsize=None)
def oracle_explicit(case, kw=()):
    """The unmodified numpy oracle on the explicit form of a shape's primed LP (computed once, shared)."""
    return solve_np(*explicit_slack_form(lp_of(case)[:7]), kw)


def emulated(lp, kw=()):
    A_ub, _, A_eq, _, c, lower, upper = lp
    _, _, _, B, F = classes(lower, upper)
    n, m = c.shape[0] + A_ub.shape[0], A_ub.shape[0] + A_eq.shape[0]
    return solve_np(*ext_form(lp), kw, solver=make_bounds_solver(n, m, B, F))


def check_against_explicit(case, kw=()):
    full = lp_of(case)
    lp = full[:7]
    ref = oracle_explicit(case, kw)
    got = emulated(lp, kw)
    assert ref.status == 0 and got.status == 0, (ref.status, got.status)
    assert got.iterations == ref.iterations, (got.iterations, ref.iterations)
    x_ref, x_got = caller_x(lp, net_of_explicit(lp, ref.x_slack)), caller_x(lp, net_of_ext(lp, got.x_slack))
    err = np.abs(x_got - x_ref).max()
    planted = np.abs(x_ref - full[7]).max()
    print(f"\n[measure] {case} {dict(kw)}: {got.iterations} iterations, max|x - x_explicit| {err:.3g}, "
          f"|fun - fun_explicit| {abs(got.fun - ref.fun):.3g}, oracle to the planted vertex {planted:.3g}")
    assert err <= X_TOL, err
    assert abs(got.fun - ref.fun) <= 1e-6 * max(1.0, abs(ref.fun))
    return planted


@pytest.mark.parametrize("case", SHAPES, ids=ids(SHAPES))
def test_emulated_algebra_matches_the_oracle_on_the_explicit_form(case):
    planted = check_against_explicit(case)
    # the oracle reaches the planted vertex: the project's tolerance on x, relative to the size of the planted values once
    # the shift has moved them away from O(1) -- a strictly complementary vertex at tol = 1e-8
    assert planted <= X_TOL * max(1.0, np.abs(lp_of(case)[7]).max()), planted


@pytest.mark.parametrize("kw", OPTIONS[1:], ids=["ip0", "tol1e-6"])
def test_emulated_algebra_under_options(kw):
    check_against_explicit(OPTION_SHAPE, kw)


def exits():
    """name -> (A_ub, b_ub, A_eq, b_eq, c, lower, upper, expected status): infeasible by its bounds (x1 + x2 + x3 = 10 inside
    [-1, 1]^3); unbounded along a free column; unbounded along a reflected column (x3 <= 2, cost +x3 ... minimised downwards);
    bounded only by a lower and an upper bound (min x1 - x2 on x1 >= -2, x2 <= 3: x = (-2, 3))."""
    z3 = np.zeros((0, 3))
    inf = np.inf
    return {
        "infeasible": (z3, np.zeros(0), np.ones((1, 3)), np.array([10.0]), np.ones(3), -np.ones(3), np.ones(3), 5),
        "unbounded_free": (z3, np.zeros(0), np.array([[1.0, 1.0, 0.0]]), np.array([1.0]), np.array([0.0, 0.0, -1.0]),
                           np.array([0.0, 0.5, -inf]), np.array([1.0, inf, inf]), 6),
        "unbounded_reflected": (z3, np.zeros(0), np.array([[1.0, 1.0, 0.0]]), np.array([1.0]), np.array([0.0, 0.0, 1.0]),
                                np.array([0.0, 0.5, -inf]), np.array([1.0, inf, 2.0]), 6),
        "by_bounds": (np.array([[1.0, 1.0]]), np.array([10.0]), np.zeros((0, 2)), np.zeros(0), np.array([1.0, -1.0]),
                      np.array([-2.0, -inf]), np.array([inf, 3.0]), 0),
    }


@pytest.mark.parametrize("name", ["infeasible", "unbounded_free", "unbounded_reflected", "by_bounds"])
def test_the_exits_behave_alike(name):
    *lp, status = exits()[name]
    lp = tuple(lp)
    ref = solve_np(*explicit_slack_form(lp))
    got = emulated(lp)
    print(f"\n[measure] {name}: status {got.status} / {ref.status}, {got.iterations} / {ref.iterations} iterations")
    assert got.status == ref.status == status
    assert got.iterations == ref.iterations
    if status == 0:
        x_ref, x_got = caller_x(lp, net_of_explicit(lp, ref.x_slack)), caller_x(lp, net_of_ext(lp, got.x_slack))
        assert np.abs(x_got - x_ref).max() <= X_TOL
        assert np.abs(x_got - np.array([-2.0, 3.0])).max() <= X_TOL


def test_symbol_and_prototype(built):
    import ctypes as C
    from lp_amd import _capi
    lib = _capi.lib()
    assert lib.lpipm_upload_bounds.restype is C.c_int
    assert len(lib.lpipm_upload_bounds.argtypes) == len(lib.lpipm_upload_bounded.argtypes) + 1 == 14
    # without a context nothing is touched: a shape without rows is Unconstrained first, then the arguments
    c = np.ones(3)
    lo, up = np.array([-1.0, -np.inf, 0.0]), np.array([1.0, np.inf, 2.0])
    cp, lp_, upp = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in (c, lo, up))
    f = lib.lpipm_upload_bounds
    assert f(None, 3, 0, None, 3, None, 0, None, 3, None, cp, 0.0, lp_, upp) == _capi.UNCONSTRAINED
    assert f(None, 3, 0, None, 3, None, 0, None, 3, None, cp, 0.0, None, None) == _capi.UNCONSTRAINED
    assert f(None, 3, 0, None, 3, None, 1, cp, 3, cp, cp, 0.0, lp_, upp) == _capi.ERR_BAD_ARGUMENT
    bad = np.array([np.nan, 0.0, 0.0])
    assert f(None, 3, 0, None, 3, None, 0, None, 3, None, cp, 0.0, bad.ctypes.data_as(C.POINTER(C.c_double)), upp) == _capi.UNCONSTRAINED


def test_builder_errors():
    import lp_amd
    cx = lp_amd.Context.__new__(lp_amd.Context)          # no device: the checks come before the library is called
    c = np.ones(3)

    def base():
        return lp_amd.Problem.target(c).ub(np.ones((2, 3)), np.ones(2))
    with pytest.raises(ValueError):
        lp_amd.Context.upload(cx, base().lower([1.0, -np.inf, 0.0]).build(), tall=True)
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        base().lower([1.0, 2.0]).build()
    for bad in (np.nan, np.inf):
        with pytest.raises(lp_amd.InvalidParameter):
            base().lower([1.0, bad, 2.0]).build()
    for bad in (np.nan, -np.inf):
        with pytest.raises(lp_amd.InvalidParameter):
            base().lower([0.0, -np.inf, 0.0]).upper([1.0, bad, 2.0]).build()
    # a lower of -inf beside a finite upper: accepted (a reflected column), and so is a free column
    p = base().lower([0.0, -np.inf, -np.inf]).upper([1.0, 2.0, np.inf]).build()
    assert p.n_bounded() == 1 and p.n_free() == 1
    assert np.array_equal(p.lower(), [0.0, -np.inf, -np.inf]) and np.array_equal(p.upper(), [1.0, 2.0, np.inf])
    # the new tail: x_slack = [x; 2 ub slacks; 1 bound slack; 1 negative part]
    xe = np.arange(7.0)
    assert np.array_equal(p.denormalize_x_into(xe), xe[:3])
    y_ub, y_eq, red = p.denormalize_duals(np.arange(3.0), xe)
    assert np.array_equal(y_ub, [0.0, 1.0]) and y_eq.shape == (0,) and np.array_equal(red, xe[:3])
    assert np.array_equal(p.denormalize_bound_duals(xe), [5.0, 0.0, 0.0])
    assert np.array_equal(p.denormalize_certificate(None, xe, 2)[2], xe[:3])
    only_lower = base().lower([1.0, 2.0, 3.0]).build()
    assert only_lower.n_bounded() == 0 and only_lower.n_free() == 0 and np.isinf(only_lower.upper()).all()


def test_builder_without_lower_builds_what_it_built_before():
    import lp_amd
    A_ub, b_ub, A_eq, b_eq, c, lower, upper, _ = lp_of(SHAPES[2])
    u = np.where(np.isfinite(upper) & np.isfinite(lower), upper - lower, np.inf)      # some finite uppers, as .upper alone takes them
    plain = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build()
    assert plain.lower() is None and plain.upper() is None and plain.n_free() == 0 and plain.n_bounded() == 0
    boxed = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).upper(u).build()
    nb = int(np.isfinite(u).sum())
    assert boxed.lower() is None and boxed.n_free() == 0 and boxed.n_bounded() == nb and np.array_equal(boxed.upper(), u)
    assert np.array_equal(boxed.A(), plain.A()) and np.array_equal(boxed.b(), plain.b()) and np.array_equal(boxed.c(), plain.c())
    xe = np.arange(float(plain.A().shape[1] + nb))
    assert np.array_equal(boxed.denormalize_x_into(xe), xe[: c.shape[0]])
    v = boxed.denormalize_bound_duals(xe)
    assert np.array_equal(v[np.isfinite(u)], xe[xe.shape[0] - nb:]) and not v[~np.isfinite(u)].any()
    # zeros for .lower: the same classes, and the upload it routes to is the one it was
    zero = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).lower(np.zeros(c.shape[0])).upper(u).build()
    assert zero.n_bounded() == nb and zero.n_free() == 0 and np.array_equal(zero._bounded, boxed._bounded)
