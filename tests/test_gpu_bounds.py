"""General column bounds (lpipm_upload_bounds): lower bounds, reflected and free columns solved on the m x m
normal equations with one stored column per free column.  Whole solves against the oracle on the explicit form of the primed LP
(free columns duplicated and negated, bound rows appended) and against lpipm_upload_ub_eq of that form, the exits, the kernel
entries against numpy / the oracle's dense sym_solve on A_ext, the passes, duals, certificates, scaling, the same bits as the
bounded form, memory, the refusals and a good solve after a failed one.
Generator, transforms, shapes and the host-side conditions on them: tests/test_bounds_host.py.  A free column's halves x+, x-
are never compared: only their difference is determined."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_bounded_host import X_TOL
from test_bounds_host import (EXPLICIT_SHAPES, OPTION_SHAPE, SHAPES, caller_x, classes, exits, explicit_parts,
                              explicit_slack_form, ext_form, ids, lp_of, net_of_explicit, primed)

pytestmark = pytest.mark.gpu

OPTION_KW = [(), (("ip", 0),), (("tol", 1e-6),)]
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def _problem(A_ub, b_ub, A_eq, b_eq, c, lower=None, upper=None):
    import lp_amd
    p = lp_amd.Problem.target(c)
    if A_ub.shape[0]:
        p = p.ub(A_ub, b_ub)
    if A_eq.shape[0]:
        p = p.eq(A_eq, b_eq)
    if lower is not None:
        p = p.lower(lower)
    if upper is not None:
        p = p.upper(upper)
    return p.build()


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _sizes(lp):
    """-> m_ub, m_eq, nx, nb, nf"""
    A_ub, _, A_eq, _, c, lower, upper = lp[:7]
    _, _, _, B, F = classes(lower, upper)
    return A_ub.shape[0], A_eq.shape[0], c.shape[0], B.shape[0], F.shape[0]


def _oracle_on(lp, kw=()):
    from oracle import capi as oracle
    ref = oracle.solve(*explicit_slack_form(lp[:7]), opts=oracle.default_opts(**dict(kw)), want_log=False)
    if ref["x_slack"] is not None:
        ref["x_slack"].setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _oracle(case, kw=()):
    """The C oracle on the explicit form of a shape's primed LP: computed once, shared, never written to."""
    return _oracle_on(lp_of(case), kw)


def _check(lp, ref, got, what):
    """The same status and iteration count; the caller's x, the `ub` slacks, w and fun to the project's bounds.  The explicit
    form's columns are [x'; x^-; ub slacks; w], the upload's [x; ub slacks; w; x^-]."""
    rc, x, fun, it, _ = got
    assert rc == ref["status"], (what, rc, ref["status"])
    assert it == ref["iterations"], (what, it, ref["iterations"])
    if ref["x_slack"] is None:
        return
    m_ub, _, nx, nb, nf = _sizes(lp)
    xr = ref["x_slack"]
    assert x.shape == (nx + m_ub + nb + nf,) and xr.shape == x.shape
    want = np.concatenate([caller_x(lp, net_of_explicit(lp, xr)), xr[nx + nf:]])
    err = np.abs(x[: nx + m_ub + nb] - want).max()
    fun_ref = ref["fun"] + primed(lp[:7])[9]               # the oracle's fun is the primed LP's: c0' = c.t
    print(f"\n[measure] {what}: status {rc}, {it} iterations, max|x - x_explicit| {err:.3g}, "
          f"fun rel {abs(fun - fun_ref) / max(1.0, abs(fun_ref)):.3g}")
    assert err <= X_TOL, (what, err)
    assert abs(fun - fun_ref) <= 1e-6 * max(1.0, abs(fun_ref)), (what, fun, fun_ref)
    assert (x[nx + m_ub + nb:] > 0).all()                  # the negative parts: interior, and nothing more is promised


# ---- 1. whole solves against the oracle on the explicit form ---------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=ids(SHAPES))
def test_solve_matches_the_oracle_on_the_explicit_form(ctx, case):
    lp = lp_of(case)
    m_ub, m_eq, nx, nb, nf = _sizes(lp)
    ctx.upload(_problem(*lp[:7]))
    assert (ctx.m, ctx.n) == (m_ub + m_eq + nb, nx + m_ub + nb + nf)
    ref = _oracle(case)
    assert ref["status"] == 0
    got = ctx.solve_raw(_opts())
    _check(lp, ref, got, f"bounds {case}")


@pytest.mark.parametrize("kw", OPTION_KW[1:], ids=["ip0", "tol1e-6"])
def test_solve_options(ctx, kw):
    lp = lp_of(OPTION_SHAPE)
    ctx.upload(_problem(*lp[:7]))
    ref = _oracle(OPTION_SHAPE, kw)
    assert ref["status"] == 0
    _check(lp, ref, ctx.solve_raw(_opts(**dict(kw))), f"bounds {OPTION_SHAPE} {kw}")


@pytest.mark.parametrize("name", ["infeasible", "unbounded_free", "unbounded_reflected", "by_bounds"])
def test_the_exits(ctx, name):
    *lp, status = exits()[name]
    ref = _oracle_on(lp)
    assert ref["status"] == status
    ctx.upload(_problem(*lp))
    got = ctx.solve_raw(_opts())
    _check(lp, ref, got, name)
    if status == 0:
        assert np.abs(got[1][:2] - np.array([-2.0, 3.0])).max() <= X_TOL


def test_the_python_solver_returns_the_callers_variables(ctx):
    import lp_amd
    case = SHAPES[2]
    lp = lp_of(case)
    res = lp_amd.InteriorPoint.default().solve(_problem(*lp[:7]))
    ref = _oracle(case)
    assert res.x().shape == lp[4].shape
    assert np.abs(res.x() - caller_x(lp, net_of_explicit(lp, ref["x_slack"]))).max() <= X_TOL
    assert abs(res.fun() - lp[4] @ res.x()) <= 1e-9 * max(1.0, abs(res.fun()))        # fun = c.x in the caller's variables


# ---- 2. against lpipm_upload_ub_eq of the explicit problem -----------------------------------------------------------------------
@pytest.mark.parametrize("case", EXPLICIT_SHAPES, ids=ids(EXPLICIT_SHAPES))
def test_bounds_agree_with_the_explicit_upload(ctx, case):
    lp = lp_of(case)
    m_ub, _, nx, nb, nf = _sizes(lp)
    o = _opts()
    ctx.upload(_problem(*explicit_parts(lp[:7])))
    old = ctx.solve_raw(o)
    ctx.upload(_problem(*lp[:7]))
    new = ctx.solve_raw(o)
    assert old[0] == 0 and new[0] == old[0] and new[3] == old[3], (old[0], new[0], old[3], new[3])
    want = np.concatenate([caller_x(lp, net_of_explicit(lp, old[1])), old[1][nx + nf:]])
    err = np.abs(new[1][: nx + m_ub + nb] - want).max()
    print(f"\n[measure] bounds vs explicit {case}: {new[3]} iterations, max|dx| {err:.3g}")
    assert err <= X_TOL, err
    fun_old = old[2] + primed(lp[:7])[9]
    assert abs(new[2] - fun_old) <= 1e-6 * max(1.0, abs(fun_old))


# ---- 3. M~ against numpy ---------------------------------------------------------------------------------------------------------
def _dtilde(dinv, n, B, F):
    nb = B.shape[0]
    dt = dinv[:n].copy()
    dt[B] = 1.0 / (1.0 / dinv[:n][B] + 1.0 / dinv[n: n + nb])
    dt[F] = dinv[:n][F] + dinv[n + nb:]
    return dt


NORMAL_SHAPES = [SHAPES[2], SHAPES[4], SHAPES[6], SHAPES[8], SHAPES[9]]


@pytest.mark.parametrize("case", NORMAL_SHAPES, ids=ids(NORMAL_SHAPES))
def test_k_bounded_normal(ctx, case):
    lp = lp_of(case)
    m_ub, m_eq, nx, nb, nf = _sizes(lp)
    _, _, _, B, F = classes(lp[5], lp[6])
    m, n = m_ub + m_eq, nx + m_ub
    ctx.upload(_problem(*lp[:7]))
    dinv = np.exp(np.random.default_rng(1000 + case[0]).uniform(-3, 3, n + nb + nf))
    M = ctx.k_bounded_normal(dinv, m)
    A = ext_form(lp[:7])[0][:m, :n]                          # A', the slack form of the primed LP
    ref = A @ (_dtilde(dinv, n, B, F)[:, None] * A.T)
    il = np.tril_indices(m)
    err = np.abs(M[il] - ref[il]).max()
    print(f"\n[measure] M~ {case}: err / (sqrt(n) max|M~|) {err / (np.sqrt(n) * np.abs(ref).max()):.3g}")
    assert err <= 1e-13 * np.sqrt(n) * np.abs(ref).max(), err          # the A.D.A^T kernel test's bound: contraction length n


# ---- 4. the reduced sym_solve against the oracle's dense one on A_ext ------------------------------------------------------------
def _iterate(rng, m, n, spread):                       # tests/test_gpu_iteration.py::_iterate
    x = np.exp(rng.uniform(-spread, spread, n)); z = np.exp(rng.uniform(-spread, spread, n))
    return x, rng.standard_normal(m), z, float(np.exp(rng.uniform(-1, 1))), float(np.exp(rng.uniform(-1, 1)))


@pytest.mark.parametrize("spread", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("case", [SHAPES[2], SHAPES[4], SHAPES[9]], ids=ids([SHAPES[2], SHAPES[4], SHAPES[9]]))
def test_k_bounded_sym_solve(ctx, case, spread):
    from oracle import oracle_np
    lp = lp_of(case)
    Ax, bx, cx = ext_form(lp[:7])
    m, n = Ax.shape
    ctx.upload(_problem(*lp[:7]))
    assert (ctx.m, ctx.n) == (m, n)
    rng = np.random.default_rng(int(10 * spread) + case[0])
    x, _, z, _, _ = _iterate(rng, m, n, spread)
    eq = oracle_np._EqSolver(Ax, x, z, 0, {"adat": 0.0, "chol": 0.0, "solves": 0.0, "gemv": 0.0})
    assert eq.ok
    pairs = [(cx, bx), (rng.standard_normal(n), rng.standard_normal(m))]          # (c, b) and a general (r1, r2)
    refs = [eq.sym_solve(Ax, r1, r2) for r1, r2 in pairs]
    rel = lambda got, ref: np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    U, V, info = ctx.k_bounded_sym_solve(x / z, np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    assert info == 0
    for q, (u, v) in enumerate(refs):
        print(f"\n[measure] sym_solve {case} spread {spread} rhs {q}: u {rel(U[q], u):.3g} v {rel(V[q], v):.3g}")
        assert rel(U[q], u) <= 1e-8 and rel(V[q], v) <= 1e-8, (q, rel(U[q], u), rel(V[q], v))     # tests/test_gpu_bounded.py's
    U1, V1, info = ctx.k_bounded_sym_solve(x / z, pairs[1][0], pairs[1][1])       # the corrector's shape: one right-hand side
    assert info == 0
    assert rel(U1[0], refs[1][0]) <= 1e-8 and rel(V1[0], refs[1][1]) <= 1e-8


@pytest.mark.parametrize("ip", [False, True])
def test_one_iteration_on_a_ext(ctx, ip):
    """One loop body (lpipm_k_iteration) against the oracle's on the dense A_ext: every F line, the net vector and the dots."""
    from oracle import capi as oracle
    from test_gpu_bounded import _compare
    case = SHAPES[2]
    lp = lp_of(case)
    Ax, bx, cx = ext_form(lp[:7])
    m, n = Ax.shape
    ctx.upload(_problem(*lp[:7]))
    rng = np.random.default_rng(100 * case[0] + int(ip))
    o = _opts()
    for trial in range(3):
        x, y, z, tau, kappa = _iterate(rng, m, n, 2.0)
        ref = oracle.iteration(Ax, bx, cx, x, y, z, tau, kappa, ip=ip)
        dev = ctx.k_iteration(o, x, y, z, tau, kappa, ip=ip)
        _compare(dev, ref)


# ---- 5. the passes see A_ext -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SHAPES[4], SHAPES[9]], ids=ids([SHAPES[4], SHAPES[9]]))
def test_passes_over_a_see_a_ext(ctx, case):
    lp = lp_of(case)
    A = ext_form(lp[:7])[0]
    m, n = A.shape
    ctx.upload(_problem(*lp[:7]))
    rng = np.random.default_rng(3)
    W, V = rng.standard_normal((2, n)), rng.standard_normal((2, m))
    tol = 1e-12 * np.sqrt(n)                              # tests/test_gpu_bounded.py::test_passes_over_a_on_a_bounded_upload
    Y, _ = ctx.k_gemv_n(W)
    assert np.abs(Y - W @ A.T).max() <= tol * max(1.0, np.abs(W @ A.T).max())
    U, _ = ctx.k_gemv_t(V)
    assert np.abs(U - V @ A).max() <= tol * max(1.0, np.abs(V @ A).max())
    Aw, ATv, _ = ctx.k_gemv_dual(W[0], V[0])
    assert np.abs(Aw - A @ W[0]).max() <= tol * max(1.0, np.abs(A @ W[0]).max())
    assert np.abs(ATv - A.T @ V[0]).max() <= tol * max(1.0, np.abs(A.T @ V[0]).max())


# ---- 6. duals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SHAPES[2], SHAPES[7]], ids=ids([SHAPES[2], SHAPES[7]]))
def test_duals_in_the_callers_orientation(ctx, case):
    import lp_amd
    lp = lp_of(case)
    A_ub, b_ub, A_eq, b_eq, c, lower, upper, xs = lp
    m_ub, m_eq, nx, nb, nf = _sizes(lp)
    sigma, _, _, B, F = classes(lower, upper)
    m, n = m_ub + m_eq, nx + m_ub
    prob = _problem(*lp[:7])
    ctx.upload(prob)
    rc, x, fun, it, _ = ctx.solve_raw(_opts())
    assert rc == 0
    d = ctx.duals()
    y, z = d["y"], d["z"]
    assert y.shape == (m + nb,) and z.shape == (n + nb + nf,)
    yb = np.zeros(nx)
    yb[B] = y[m:]
    res = np.abs(A_ub.T @ y[:m_ub] + A_eq.T @ y[m_ub:m] + yb + z[:nx] - c).max()      # A^T y + z = c, the caller's A and c
    N = sigma < 0
    print(f"\n[measure] duals {case}: |A^T y + z - c| {res:.3g}, max z on N {z[:nx][N].max(initial=-np.inf):.3g}, "
          f"max|z| on F {np.abs(z[:nx][F]).max(initial=0):.3g}, max y_b {y[m:].max(initial=-np.inf):.3g}")
    assert res <= X_TOL
    assert (z[:nx][N] <= X_TOL).all() and (z[:nx][~N] >= -X_TOL).all()
    assert np.abs(z[:nx][F]).max(initial=0) <= X_TOL
    assert (y[m:] <= X_TOL).all()
    assert (z[nx:] >= 0).all()                                                        # slacks, v, z^-: the iterate's own
    assert abs(d["dual_fun"] - fun) <= 1e-6 * max(1.0, abs(fun))
    out = lp_amd.InteriorPoint.default().solve_uploaded(ctx, prob, want_duals=True)
    assert out.reduced_costs.shape == c.shape and out.upper.shape == c.shape
    assert np.abs(c - A_ub.T @ out.y_ub - A_eq.T @ out.y_eq + out.upper - out.reduced_costs).max() <= X_TOL
    assert np.abs(out.x() - xs).max() <= X_TOL * max(1.0, np.abs(xs).max())      # the planted vertex, as tests/test_bounds_host.py has it


# ---- 7. certificates -------------------------------------------------------------------------------------------------------------
def test_certificates_satisfy_the_headers_identities(ctx):
    from lp_amd import _capi
    *lp, status = exits()["infeasible"]
    A_ub, b_ub, A_eq, b_eq, c, lower, upper = lp
    sigma, t, up, B, F = classes(lower, upper)
    Ax, bx, cx = ext_form(lp)                                # (b' = b - A.t recomputed in numpy: bx = [b'; u'])
    ctx.upload(_problem(*lp))
    assert ctx.solve_raw(_opts())[0] == status
    cert = ctx.certificate()
    assert cert["kind"] == _capi.CERT_FARKAS
    y, z = cert["y"], cert["col"].copy()
    z[: c.shape[0]] *= sigma                                 # back to the primed orientation: z' = sigma z
    assert abs(bx @ y - 1.0) <= X_TOL and (z >= 0).all()
    assert np.abs(Ax.T @ y + z).max() <= X_TOL and cert["residual"] <= X_TOL and cert["scale"] > 0
    for name in ("unbounded_free", "unbounded_reflected"):
        *lp, status = exits()[name]
        A_ub, b_ub, A_eq, b_eq, c, lower, upper = lp
        sigma, t, up, B, F = classes(lower, upper)
        nx = c.shape[0]
        ctx.upload(_problem(*lp))
        assert ctx.solve_raw(_opts())[0] == status
        cert = ctx.certificate()
        assert cert["kind"] == _capi.CERT_RAY and cert["y"] is None
        x = cert["col"][:nx]
        assert abs(c @ x + 1.0) <= X_TOL, name                                        # c.x = -1 in the caller's orientation
        assert np.abs(A_eq @ x).max(initial=0) <= X_TOL and cert["residual"] <= X_TOL and cert["scale"] > 0
        N = sigma < 0
        free = np.zeros(nx, dtype=bool)
        free[F] = True
        assert (x[~N & ~free] >= 0).all() and (x[N] <= 0).all(), name
        assert x[2] < 0 if name == "unbounded_reflected" else x[2] > 0


# ---- 8. scaling ------------------------------------------------------------------------------------------------------------------
def test_scaling_returns_the_callers_units(built):
    import lp_amd
    case = SHAPES[7]
    lp = lp_of(case)
    A_ub, b_ub, A_eq, b_eq, c, lower, upper, _ = lp
    m_ub, m_eq, nx, nb, nf = _sizes(lp)
    _, _, _, B, F = classes(lower, upper)
    m, n = m_ub + m_eq, nx + m_ub
    rng = np.random.default_rng(44)
    er, ec = rng.integers(-8, 9, m).astype(np.int32), rng.integers(-8, 9, nx).astype(np.int32)
    Aud, Aed = np.ldexp(A_ub, er[:m_ub, None] + ec[None, :]), np.ldexp(A_eq, er[m_ub:, None] + ec[None, :])
    bud, bed, cd = np.ldexp(b_ub, er[:m_ub]), np.ldexp(b_eq, er[m_ub:]), np.ldexp(c, ec)
    lod, upd = np.ldexp(lower, -ec), np.ldexp(upper, -ec)                         # optimum: ldexp(x*, -ec)
    cx = lp_amd.Context(0).set_scaling(8)
    cx.upload(_problem(Aud, bud, Aed, bed, cd, lod, upd))
    kr, kc = cx.scaling()
    assert kr.shape == (m + nb,) and kc.shape == (n + nb + nf,)
    assert np.array_equal(kc[nx:n], -kr[:m_ub])                                   # the `ub` slacks, as on any upload
    assert np.array_equal(kr[m:], -kc[B]) and np.array_equal(kc[n: n + nb], kc[B])    # the bound rows and their slack columns
    assert np.array_equal(kc[n + nb:], kc[F])                                     # every x^- column has its column's exponent
    assert np.any(kr[:m] != 0) and np.any(kc[:nx] != 0)
    got = cx.solve_raw(_opts())
    cx.close()
    ref = _oracle(case)                                                           # the unscaled solve's oracle
    assert got[0] == 0 == ref["status"]
    err = np.abs(np.ldexp(got[1][:nx], ec) - caller_x(lp, net_of_explicit(lp, ref["x_slack"]))).max()
    print(f"\n[measure] scaled {case}: {got[3]} iterations (oracle, unscaled: {ref['iterations']}), max|x - x_oracle| {err:.3g}")
    assert err <= X_TOL, err


# ---- 9. the same bits as the bounded form ----------------------------------------------------------------------------------------
def _raw_solve(upload, m, n):
    """A fresh context, `upload(handle)`, one solve -> (solve_raw's tuple, duals y, duals z, resident bytes)"""
    import lp_amd
    cx = lp_amd.Context(0)
    assert upload(cx._h) == 0
    cx.m, cx.n = m, n
    got = cx.solve_raw(_opts())
    d = cx.duals()
    out = (got, d["y"], d["z"], cx.resident_bytes())
    cx.close()
    return out


@pytest.mark.parametrize("which", ["zeros-finite", "null-finite", "zeros-inf", "null-null"])
def test_zero_lowers_are_the_bounded_form_bit_for_bit(built, which):
    from lp_amd import _capi
    from test_bounded_host import planted_box
    L = _capi.lib()
    lo, finite = which.split("-")
    # (without finite uppers: a vertex no bound takes part in, as tests/test_gpu_bounded.py's nb == 0 test has it)
    A_ub, b_ub, A_eq, b_eq, c, u, _ = planted_box(3, 20, 4, 60, .5 if finite == "finite" else 0, .5)
    m_ub, m_eq, nx = A_ub.shape[0], A_eq.shape[0], c.shape[0]
    lower = np.zeros(nx) if lo == "zeros" else None
    upper = u if finite == "finite" else (np.full(nx, np.inf) if finite == "inf" else None)
    nb = int(np.isfinite(upper).sum()) if upper is not None else 0
    m, n = m_ub + m_eq + nb, nx + m_ub + nb
    args = (nx, m_ub, dp(A_ub), nx, dp(b_ub), m_eq, dp(A_eq), nx, dp(b_eq), dp(c), 0.0)
    new = _raw_solve(lambda h: L.lpipm_upload_bounds(h, *args, dp(lower) if lower is not None else None,
                                                     dp(upper) if upper is not None else None), m, n)
    if finite == "null":
        old = _raw_solve(lambda h: L.lpipm_upload_ub_eq(h, *args), m, n)
    else:
        old = _raw_solve(lambda h: L.lpipm_upload_bounded(h, *args, dp(upper)), m, n)
    assert old[0][0] == 0 and new[0][0] == 0 and new[0][3] == old[0][3] and new[3] == old[3]
    assert _bits(new[0][1]) == _bits(old[0][1]) and _bits(new[0][2]) == _bits(old[0][2])
    assert _bits(new[1]) == _bits(old[1]) and _bits(new[2]) == _bits(old[2])


# ---- 10. memory ------------------------------------------------------------------------------------------------------------------
def test_resident_bytes_grow_with_n_plus_nf_not_with_a_copy_of_the_free_columns(built):
    import lp_amd
    _, m_ub, m_eq, nx = SHAPES[6][:4]                        # shape 7's sizes, every column free
    rng = np.random.default_rng(7)
    A_ub, A_eq, c = rng.standard_normal((m_ub, nx)), rng.standard_normal((m_eq, nx)), rng.standard_normal(nx)
    b_ub, b_eq = rng.standard_normal(m_ub), rng.standard_normal(m_eq)
    free = (np.full(nx, -np.inf), np.full(nx, np.inf))
    sizes = {}
    # (the baseline is the same form with every column merely shifted: an x >= 0 upload also keeps a first factor, m x m more)
    for name, prob in (("shifted", _problem(A_ub, b_ub, A_eq, b_eq, c, np.ones(nx))), ("free", _problem(A_ub, b_ub, A_eq, b_eq, c, *free)),
                       ("split", _problem(np.hstack([A_ub, -A_ub]), b_ub, np.hstack([A_eq, -A_eq]), b_eq, np.concatenate([c, -c])))):
        cx = lp_amd.Context(0)
        cx.upload(prob)
        sizes[name] = cx.resident_bytes()
        cx.close()
    print(f"\n[measure] resident bytes at shape 7, every column free: {sizes}")
    assert sizes["free"] < sizes["split"], sizes
    # what the free columns add: the nf longer column vectors (12 iterate and work vectors, two rows of W, xout: < 20 doubles
    # an entry), the net vector and the free columns' lists over the n columns (< 3 doubles an entry), and page rounding (every
    # length padded to 256) -- against 8 m nf bytes for a second copy of A_F
    n, nf, m = nx + m_ub, nx, m_ub + m_eq
    grown = sizes["free"] - sizes["shifted"]
    assert 0 < grown <= 8 * (20 * (nf + 256) + 3 * (n + 256)) + 3 * 4096, (grown, sizes)
    assert grown < 8 * m * nf / 2, (grown, 8 * m * nf)


# ---- 11. refusals ----------------------------------------------------------------------------------------------------------------
class _NeverCalled:
    """An all-reduce for lpipm_set_collective that no refused upload may reach."""
    def __init__(self):
        from lp_amd import _capi
        self.calls = 0
        self.cfn = _capi.ALLREDUCE_FN(self._call)

    def _call(self, *args):
        self.calls += 1
        return 1


def test_refusals(built, monkeypatch):
    import lp_amd
    from lp_amd import _capi
    L = _capi.lib()
    lp = lp_of(SHAPES[2])
    A_ub, b_ub, A_eq, b_eq, c, lower, upper, _ = lp
    m_ub, m_eq, nx, nb, nf = _sizes(lp)
    m, n = m_ub + m_eq + nb, nx + m_ub + nb + nf
    up = lambda h, lo, hi: L.lpipm_upload_bounds(h, nx, m_ub, dp(A_ub), nx, dp(b_ub), m_eq, dp(A_eq), nx, dp(b_eq), dp(c), 0.0,
                                                 dp(lo), dp(hi))
    cx = lp_amd.Context(0)
    cx.upload(_problem(*lp[:7]))
    want = cx.solve_raw(_opts())
    assert want[0] == 0

    def unchanged():
        again = cx.solve_raw(_opts())
        assert again[0] == 0 and again[3] == want[3] and _bits(again[1]) == _bits(want[1]) and _bits(again[2]) == _bits(want[2])

    for lo_bad, hi_bad in ((np.nan, None), (np.inf, None), (None, np.nan), (None, -np.inf)):
        lo, hi = lower.copy(), upper.copy()
        if lo_bad is not None:
            lo[1] = lo_bad
        if hi_bad is not None:
            hi[1] = hi_bad
        assert up(cx._h, lo, hi) == _capi.ERR_BAD_ARGUMENT, (lo_bad, hi_bad)
        unchanged()
    lo, hi = lower.copy(), upper.copy()
    lo[1], hi[1] = 2.0, 1.0                                   # crossed: no point satisfies the bounds
    assert up(cx._h, lo, hi) == _capi.INFEASIBLE
    unchanged()
    assert L.lpipm_upload_bounds(cx._h, nx, 0, None, nx, None, 0, None, nx, None, dp(c), 0.0, dp(lower), dp(upper)) == _capi.UNCONSTRAINED
    unchanged()
    for st in (1, 2):
        assert cx.solve_raw(_opts(solver_type=st))[0] == _capi.ERR_UNSUPPORTED
    unchanged()
    bs, cs = np.ones(m), np.ones(n)
    assert L.lpipm_update_vectors(cx._h, dp(bs), dp(cs)) == _capi.ERR_UNSUPPORTED
    unchanged()
    d, M = np.ones(n), np.empty((m, m))
    assert L.lpipm_k_adat(cx._h, dp(d), dp(M), 1, None) == _capi.ERR_UNSUPPORTED
    unchanged()
    cx.close()
    # a column-split context and one with the refined solves
    split = lp_amd.Context(0)
    coll = _NeverCalled()
    split.set_collective(1, 2, coll)
    assert up(split._h, lower, upper) == _capi.ERR_UNSUPPORTED
    assert split.resident_bytes() == 0 and coll.calls == 0
    split.close()
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_REFINE", "2")
    refining = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_REFINE")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    assert up(refining._h, lower, upper) == _capi.ERR_UNSUPPORTED
    assert refining.resident_bytes() == 0
    refining.close()
    # the Python upload raises what the library returns
    with pytest.raises(lp_amd.Infeasible):
        lp_amd.Context(0).upload(_problem(A_ub, b_ub, A_eq, b_eq, c, lo, hi))


def test_equal_ends_are_a_bound_of_width_zero(ctx):
    """lower_j == upper_j is class B with u' = 0: accepted, and it behaves as the explicit form does (whatever that is)."""
    *lp, _ = exits()["by_bounds"]
    A_ub, b_ub, A_eq, b_eq, c, lower, upper = lp
    lower, upper = lower.copy(), upper.copy()
    lower[1] = upper[1] = 3.0
    lp = (A_ub, b_ub, A_eq, b_eq, c, lower, upper)
    ref = _oracle_on(lp)
    ctx.upload(_problem(*lp))
    got = ctx.solve_raw(_opts())
    assert got[0] == ref["status"] and got[3] == ref["iterations"]


# ---- 12. a good solve after a failed one -----------------------------------------------------------------------------------------
def test_a_good_solve_after_a_failed_one_has_the_good_ones_bits(built):
    import lp_amd
    from lp_amd import _capi
    lp = lp_of(SHAPES[2])
    good = _problem(*lp[:7])
    *bad, status = exits()["infeasible"]
    fresh = lp_amd.Context(0)
    fresh.upload(good)
    want = fresh.solve_raw(_opts())
    fresh.close()
    assert want[0] == 0
    cx = lp_amd.Context(0)
    cx.upload(good)
    assert cx.solve_raw(_opts(max_iter=2))[0] == _capi.ITERATION_LIMIT        # stopped half way: the iterate is left mid-solve
    again = cx.solve_raw(_opts())
    assert again[0] == 0 and again[3] == want[3] and _bits(again[1]) == _bits(want[1]) and _bits(again[2]) == _bits(want[2])
    cx.upload(_problem(*bad))
    assert cx.solve_raw(_opts())[0] == status                                 # an infeasible upload on the same context
    cx.upload(good)
    after = cx.solve_raw(_opts())
    cx.upload(_problem(*lp[:5]))                                              # ... and nothing of the form leaks into a plain one
    plain_after = cx.solve_raw(_opts())
    cx.close()
    assert after[0] == 0 and after[3] == want[3] and _bits(after[1]) == _bits(want[1]) and _bits(after[2]) == _bits(want[2])
    plain = lp_amd.Context(0)
    plain.upload(_problem(*lp[:5]))
    plain_want = plain.solve_raw(_opts())
    plain.close()
    assert plain_after[0] == plain_want[0] and plain_after[3] == plain_want[3]
    assert _bits(plain_after[1]) == _bits(plain_want[1]) and _bits(plain_after[2]) == _bits(plain_want[2])
