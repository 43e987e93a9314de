"""The bounded form (lpipm_upload_bounded): upper bounds on structural columns solved on the m x m normal
equations.  Whole solves against the oracle on the explicit form (the bound rows appended to the `ub` rows) and against
lpipm_upload_ub_eq of that form, the three exits, the kernel entries against numpy / the oracle's dense sym_solve and loop body
on A_ext, the passes, duals, certificates, nb == 0, scaling, memory, the refusals and what a bounded solve leaves behind.
Generator, shapes and the host-side conditions on them: tests/test_bounded_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_bounded_host import (EXPLICIT_SHAPES, OPTION_SHAPE, SHAPES, X_TOL, bounded_columns, exits, explicit_parts,
                               explicit_slack_form, ext_form, ids, planted_box)

pytestmark = pytest.mark.gpu

OPTION_KW = [(), (("ip", 0),), (("tol", 1e-6),)]
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def _problem(A_ub, b_ub, A_eq, b_eq, c, u=None):
    import lp_amd
    p = lp_amd.Problem.target(c)
    if A_ub.shape[0]:
        p = p.ub(A_ub, b_ub)
    if A_eq.shape[0]:
        p = p.eq(A_eq, b_eq)
    return (p.upper(u) if u is not None else p).build()


def _explicit_problem(A_ub, b_ub, A_eq, b_eq, c, u):
    Au, bu = explicit_parts(A_ub, b_ub, u)
    return _problem(Au, bu, A_eq, b_eq, c)


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _oracle(case, kw=()):
    """The C oracle on the explicit form of a shape: computed once, shared, never written to."""
    from oracle import capi as oracle
    ref = oracle.solve(*explicit_slack_form(*planted_box(*case)[:6]), opts=oracle.default_opts(**dict(kw)), want_log=False)
    if ref["x_slack"] is not None:
        ref["x_slack"].setflags(write=False)
    return ref


def _check(ref, got, what):
    """The same status and iteration count; x over all n + m_ub + nb entries and fun to the project's bounds."""
    rc, x, fun, it, _ = got
    assert rc == ref["status"], (what, rc, ref["status"])
    assert it == ref["iterations"], (what, it, ref["iterations"])
    if ref["x_slack"] is not None:
        assert x.shape == ref["x_slack"].shape
        err = np.abs(x - ref["x_slack"]).max()
        print(f"\n[measure] {what}: status {rc}, {it} iterations, max|x - x_explicit| {err:.3g}, "
              f"fun rel {abs(fun - ref['fun']) / max(1.0, abs(ref['fun'])):.3g}")
        assert err <= X_TOL, (what, err)
        assert abs(fun - ref["fun"]) <= 1e-6 * max(1.0, abs(ref["fun"])), (what, fun, ref["fun"])


def _lengths(lp):
    A_ub, _, A_eq, _, c, u = lp[:6]
    nb = bounded_columns(u).shape[0]
    return A_ub.shape[0] + A_eq.shape[0] + nb, c.shape[0] + A_ub.shape[0] + nb, nb


# ---- 1. whole solves against the oracle on the explicit form ---------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPES, ids=ids(SHAPES))
def test_solve_matches_the_oracle_on_the_explicit_form(ctx, case):
    lp = planted_box(*case)
    ctx.upload(_problem(*lp[:6]))
    assert (ctx.m, ctx.n) == _lengths(lp)[:2]
    ref = _oracle(case)
    assert ref["status"] == 0
    _check(ref, ctx.solve_raw(_opts()), f"bounded {case}")


@pytest.mark.parametrize("kw", OPTION_KW[1:], ids=["ip0", "tol1e-6"])
def test_solve_options(ctx, kw):
    lp = planted_box(*OPTION_SHAPE)
    ctx.upload(_problem(*lp[:6]))
    ref = _oracle(OPTION_SHAPE, kw)
    assert ref["status"] == 0
    _check(ref, ctx.solve_raw(_opts(**dict(kw))), f"bounded {OPTION_SHAPE} {kw}")


@pytest.mark.parametrize("name", ["infeasible", "unbounded", "by_bounds"])
def test_the_three_exits(ctx, name):
    from oracle import capi as oracle
    *lp, status = exits()[name]
    ref = oracle.solve(*explicit_slack_form(*lp), want_log=False)
    assert ref["status"] == status
    ctx.upload(_problem(*lp))
    got = ctx.solve_raw(_opts())
    _check(ref, got, name)
    if status == 0:
        assert np.abs(got[1][:2] - np.array([3.0, 2.0])).max() <= X_TOL


# ---- 2. against lpipm_upload_ub_eq of the explicit problem -----------------------------------------------------------------------
@pytest.mark.parametrize("case", EXPLICIT_SHAPES, ids=ids(EXPLICIT_SHAPES))
def test_bounded_agrees_with_the_explicit_upload(ctx, case):
    lp = planted_box(*case)
    o = _opts()
    ctx.upload(_explicit_problem(*lp[:6]))
    old = ctx.solve_raw(o)
    ctx.upload(_problem(*lp[:6]))
    new = ctx.solve_raw(o)
    assert old[0] == 0 and new[0] == old[0] and new[3] == old[3], (old[0], new[0], old[3], new[3])
    err = np.abs(new[1] - old[1]).max()
    print(f"\n[measure] bounded vs explicit {case}: {new[3]} iterations, max|dx| {err:.3g}")
    assert err <= X_TOL, err
    assert abs(new[2] - old[2]) <= 1e-6 * max(1.0, abs(old[2]))


# ---- 3. M~ against numpy ---------------------------------------------------------------------------------------------------------
def _dtilde(dinv, n, B):
    dt = dinv[:n].copy()
    dt[B] = 1.0 / (1.0 / dinv[:n][B] + 1.0 / dinv[n:])
    return dt


@pytest.mark.parametrize("case", [SHAPES[2], SHAPES[4], SHAPES[6], SHAPES[8]], ids=ids([SHAPES[2], SHAPES[4], SHAPES[6], SHAPES[8]]))
def test_k_bounded_normal(ctx, case):
    lp = planted_box(*case)
    A_ub, _, A_eq, _, c, u = lp[:6]
    m_ext, n_ext, nb = _lengths(lp)
    m, n = m_ext - nb, n_ext - nb
    ctx.upload(_problem(*lp[:6]))
    dinv = np.exp(np.random.default_rng(1000 + case[0]).uniform(-3, 3, n_ext))
    M = ctx.k_bounded_normal(dinv, m)
    A = ext_form(*lp[:6])[0][:m, :n]
    ref = A @ (_dtilde(dinv, n, bounded_columns(u))[:, None] * A.T)
    il = np.tril_indices(m)
    err = np.abs(M[il] - ref[il]).max()
    print(f"\n[measure] M~ {case}: err / (sqrt(n) max|M~|) {err / (np.sqrt(n) * np.abs(ref).max()):.3g}")
    assert err <= 1e-13 * np.sqrt(n) * np.abs(ref).max(), err          # the A.D.A^T kernel test's bound: contraction length n


# ---- 4. the reduced sym_solve against the oracle's dense one on A_ext ------------------------------------------------------------
def _iterate(rng, m, n, spread):                       # tests/test_gpu_iteration.py::_iterate
    x = np.exp(rng.uniform(-spread, spread, n)); z = np.exp(rng.uniform(-spread, spread, n))
    return x, rng.standard_normal(m), z, float(np.exp(rng.uniform(-1, 1))), float(np.exp(rng.uniform(-1, 1)))


@pytest.mark.parametrize("spread", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("case", [SHAPES[2], SHAPES[4]], ids=ids([SHAPES[2], SHAPES[4]]))
def test_k_bounded_sym_solve(ctx, case, spread):
    from oracle import oracle_np
    lp = planted_box(*case)
    Ax, bx, cx = ext_form(*lp[:6])
    m, n = Ax.shape
    ctx.upload(_problem(*lp[:6]))
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
        assert rel(U[q], u) <= 1e-8 and rel(V[q], v) <= 1e-8, (q, rel(U[q], u), rel(V[q], v))
    U1, V1, info = ctx.k_bounded_sym_solve(x / z, pairs[1][0], pairs[1][1])       # the corrector's shape: one right-hand side
    assert info == 0
    assert rel(U1[0], refs[1][0]) <= 1e-8 and rel(V1[0], refs[1][1]) <= 1e-8


# ---- 5. one loop body against oracle.iteration on A_ext --------------------------------------------------------------------------
def _compare(dev, ref):                               # tests/test_gpu_tall_form.py::_compare
    assert ref["status"] == 0 and dev["info"] == 0
    scale = lambda a: max(1.0, np.abs(a).max())
    for k in ("d_x", "d_y", "d_z"):
        assert np.abs(dev[k] - ref[k]).max() <= 1e-8 * scale(ref[k]), k
    for k in ("d_tau", "d_kappa"):
        assert abs(dev[k] - ref[k]) <= 1e-8 * max(1.0, abs(ref[k])), k
    assert abs(dev["alpha"] - ref["alpha"]) <= 1e-8
    for k in ("x", "y", "z"):
        assert np.abs(dev[k] - ref[k]).max() <= 1e-8 * scale(ref[k]), k
    assert abs(dev["tau"] - ref["tau"]) <= 1e-8 * max(1.0, abs(ref["tau"]))
    assert abs(dev["kappa"] - ref["kappa"]) <= 1e-8 * max(1.0, abs(ref["kappa"]))


@pytest.mark.parametrize("case,spread", [(SHAPES[1], 1.0), (SHAPES[2], 2.0), (SHAPES[4], 1.5)], ids=ids([SHAPES[1], SHAPES[2], SHAPES[4]]))
@pytest.mark.parametrize("ip", [False, True])
def test_one_iteration_on_a_bounded_upload(ctx, case, spread, ip):
    from oracle import capi as oracle
    lp = planted_box(*case)
    Ax, bx, cx = ext_form(*lp[:6])
    m, n = Ax.shape
    ctx.upload(_problem(*lp[:6]))
    rng = np.random.default_rng(100 * case[0] + int(ip))
    o = _opts()
    for trial in range(4):
        x, y, z, tau, kappa = _iterate(rng, m, n, spread)
        ref = oracle.iteration(Ax, bx, cx, x, y, z, tau, kappa, ip=ip)
        dev = ctx.k_iteration(o, x, y, z, tau, kappa, ip=ip)
        _compare(dev, ref)


# ---- 6. the passes see A_ext -----------------------------------------------------------------------------------------------------
def test_passes_over_a_on_a_bounded_upload(ctx):
    lp = planted_box(*SHAPES[4])
    A = ext_form(*lp[:6])[0]
    m, n = A.shape
    ctx.upload(_problem(*lp[:6]))
    rng = np.random.default_rng(3)
    W, V = rng.standard_normal((2, n)), rng.standard_normal((2, m))
    tol = 1e-12 * np.sqrt(n)                              # tests/test_gpu_tall_form.py::test_passes_over_a_on_a_tall_upload
    Y, _ = ctx.k_gemv_n(W)
    assert np.abs(Y - W @ A.T).max() <= tol * max(1.0, np.abs(W @ A.T).max())
    U, _ = ctx.k_gemv_t(V)
    assert np.abs(U - V @ A).max() <= tol * max(1.0, np.abs(V @ A).max())
    Aw, ATv, _ = ctx.k_gemv_dual(W[0], V[0])
    assert np.abs(Aw - A @ W[0]).max() <= tol * max(1.0, np.abs(A @ W[0]).max())
    assert np.abs(ATv - A.T @ V[0]).max() <= tol * max(1.0, np.abs(A.T @ V[0]).max())


# ---- 7. duals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SHAPES[2], SHAPES[7]], ids=ids([SHAPES[2], SHAPES[7]]))
def test_duals_of_a_bounded_solve(ctx, case):
    import lp_amd
    lp = planted_box(*case)
    A_ub, b_ub, A_eq, b_eq, c, u = lp[:6]
    Ax, bx, cx = ext_form(*lp[:6])
    m, n = Ax.shape
    nb = bounded_columns(u).shape[0]
    prob = _problem(*lp[:6])
    ctx.upload(prob)
    rc, x, fun, it, _ = ctx.solve_raw(_opts())
    assert rc == 0
    d = ctx.duals()
    y, z = d["y"], d["z"]
    assert y.shape == (m,) and z.shape == (n,)
    res = np.abs(Ax.T @ y + z - cx).max()
    print(f"\n[measure] duals {case}: |A_ext^T y + z - c_ext| {res:.3g}, max y_b {y[m - nb:].max():.3g}, |y_b + v| {np.abs(y[m - nb:] + z[n - nb:]).max():.3g}")
    assert res <= X_TOL and (z >= 0).all()
    assert (y[m - nb:] <= X_TOL).all()                           # a bound row's multiplier is <= 0 up to the dual residual
    assert np.abs(y[m - nb:] + z[n - nb:]).max() <= X_TOL        # ... and equals -v
    assert abs(d["dual_fun"] - fun) <= 1e-6 * max(1.0, abs(fun))
    out = lp_amd.InteriorPoint.default().solve_uploaded(ctx, prob, want_duals=True)
    v = out.upper
    assert v.shape == c.shape and not v[~np.isfinite(u)].any() and (v >= 0).all()
    assert np.abs(c - A_ub.T @ out.y_ub - A_eq.T @ out.y_eq + v - out.reduced_costs).max() <= X_TOL
    assert np.abs(out.x() - lp[6]).max() <= X_TOL


# ---- 8. certificates -------------------------------------------------------------------------------------------------------------
def test_certificates_of_the_bounded_exits(ctx):
    from lp_amd import _capi
    *lp, status = exits()["infeasible"]
    Ax, bx, cx = ext_form(*lp)
    ctx.upload(_problem(*lp))
    assert ctx.solve_raw(_opts())[0] == status
    cert = ctx.certificate()
    assert cert["kind"] == _capi.CERT_FARKAS
    y, z = cert["y"], cert["col"]
    assert abs(bx @ y - 1.0) <= X_TOL and (z >= 0).all()
    assert np.abs(Ax.T @ y + z).max() <= X_TOL and cert["residual"] <= X_TOL and cert["scale"] > 0
    *lp, status = exits()["unbounded"]
    Ax, bx, cx = ext_form(*lp)
    ctx.upload(_problem(*lp))
    assert ctx.solve_raw(_opts())[0] == status
    cert = ctx.certificate()
    assert cert["kind"] == _capi.CERT_RAY and cert["y"] is None
    x = cert["col"]
    assert abs(cx @ x + 1.0) <= X_TOL and (x >= 0).all()
    assert np.abs(Ax @ x).max() <= X_TOL and cert["residual"] <= X_TOL and cert["scale"] > 0


# ---- 9. nb == 0 is lpipm_upload_ub_eq --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upper", ["null", "inf"])
def test_without_a_finite_bound_it_is_upload_ub_eq(built, upper):
    import lp_amd
    from lp_amd import _capi
    A_ub, b_ub, A_eq, b_eq, c, u, _ = planted_box(3, 20, 4, 60, 0, .5)           # (frac 0: a vertex no bound takes part in)
    m_ub, m_eq, nx = A_ub.shape[0], A_eq.shape[0], c.shape[0]
    assert np.isinf(u).all()
    got = []
    for bounded in (False, True):
        cx = lp_amd.Context(0)
        if bounded:
            rc = _capi.lib().lpipm_upload_bounded(cx._h, nx, m_ub, dp(A_ub), nx, dp(b_ub), m_eq, dp(A_eq), nx, dp(b_eq), dp(c), 0.0,
                                                  dp(u) if upper == "inf" else None)
        else:
            rc = _capi.lib().lpipm_upload_ub_eq(cx._h, nx, m_ub, dp(A_ub), nx, dp(b_ub), m_eq, dp(A_eq), nx, dp(b_eq), dp(c), 0.0)
        assert rc == 0
        cx.m, cx.n = m_ub + m_eq, nx + m_ub
        got.append((cx.solve_raw(_opts()), cx.resident_bytes()))
        cx.close()
    (old, old_bytes), (new, new_bytes) = got
    assert old[0] == 0 and new[0] == 0 and new[3] == old[3] and new_bytes == old_bytes
    assert _bits(new[1]) == _bits(old[1]) and _bits(new[2]) == _bits(old[2])


# ---- 10. scaling -----------------------------------------------------------------------------------------------------------------
def test_scaling_is_the_host_scaled_solve(built):
    import lp_amd
    case = SHAPES[7]
    A_ub, b_ub, A_eq, b_eq, c, u, xs = planted_box(*case)
    m_ub, m_eq, nx = A_ub.shape[0], A_eq.shape[0], c.shape[0]
    B = bounded_columns(u)
    nb, m, n = B.shape[0], m_ub + m_eq, nx + m_ub
    rng = np.random.default_rng(44)
    er, ec = rng.integers(-8, 9, m).astype(np.int32), rng.integers(-8, 9, nx).astype(np.int32)
    Aud, Aed = np.ldexp(A_ub, er[:m_ub, None] + ec[None, :]), np.ldexp(A_eq, er[m_ub:, None] + ec[None, :])
    bud, bed, cd, ud = np.ldexp(b_ub, er[:m_ub]), np.ldexp(b_eq, er[m_ub:]), np.ldexp(c, ec), np.ldexp(u, -ec)   # optimum: ldexp(x*, -ec)
    o = _opts()
    cx = lp_amd.Context(0).set_scaling(8)
    cx.upload(_problem(Aud, bud, Aed, bed, cd, ud))
    kr, kc = cx.scaling()
    assert kr.shape == (m + nb,) and kc.shape == (n + nb,)
    assert np.array_equal(kc[nx:n], -kr[:m_ub])                                   # the `ub` slacks, as on any upload
    assert np.array_equal(kr[m:], -kc[B]) and np.array_equal(kc[n:], kc[B])       # the bound rows and their slack columns
    assert np.any(kr[:m] != 0) and np.any(kc[:nx] != 0)
    got = cx.solve_raw(o, want_log=True)
    cx.close()
    ref_cx = lp_amd.Context(0)
    ref_cx.upload(_problem(np.ldexp(Aud, kr[:m_ub, None] + kc[None, :nx]), np.ldexp(bud, kr[:m_ub]),
                           np.ldexp(Aed, kr[m_ub:m, None] + kc[None, :nx]), np.ldexp(bed, kr[m_ub:m]), np.ldexp(cd, kc[:nx]),
                           np.ldexp(ud, -kc[:nx])))
    ref = ref_cx.solve_raw(o, want_log=True)
    ref_cx.close()
    # tests/test_gpu_scaling.py's criterion: status, count, every log row and fun bit for bit, x = ldexp(x_ref, kc) bit for bit
    assert got[0] == 0 and got[0] == ref[0] and got[3] == ref[3]
    assert _bits(got[1]) == _bits(np.ldexp(ref[1], kc))
    assert _bits(got[2]) == _bits(ref[2])
    assert len(got[4]) == len(ref[4]) and _bits(np.array(got[4])) == _bits(np.array(ref[4]))
    assert np.abs(np.ldexp(got[1][:nx], ec) - xs).max() <= X_TOL                  # ... and x is in the caller's units


# ---- 11. memory ------------------------------------------------------------------------------------------------------------------
def test_resident_bytes_stay_those_of_the_m_by_m_system(built):
    import lp_amd
    lp = planted_box(11, 0, 128, 512, 1, .5)
    sizes = {}
    for name, prob in (("bounded", _problem(*lp[:6])), ("explicit", _explicit_problem(*lp[:6]))):
        cx = lp_amd.Context(0)
        cx.upload(prob)
        sizes[name] = cx.resident_bytes()
        cx.close()
    print(f"\n[measure] resident bytes at 128 x 512, every column bounded: {sizes}")
    assert sizes["bounded"] < sizes["explicit"], sizes       # a 128^2 system against a 640^2 one


# ---- 12. refusals ----------------------------------------------------------------------------------------------------------------
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
    A_ub, b_ub, A_eq, b_eq, c, u, _ = planted_box(*SHAPES[2])
    m_ub, m_eq, nx = A_ub.shape[0], A_eq.shape[0], c.shape[0]
    nb = bounded_columns(u).shape[0]
    m, n = m_ub + m_eq + nb, nx + m_ub + nb
    up = lambda h, uu: L.lpipm_upload_bounded(h, nx, m_ub, dp(A_ub), nx, dp(b_ub), m_eq, dp(A_eq), nx, dp(b_eq), dp(c), 0.0, dp(uu))
    cx = lp_amd.Context(0)
    cx.upload(_problem(A_ub, b_ub, A_eq, b_eq, c, u))
    want = cx.solve_raw(_opts())
    assert want[0] == 0

    def unchanged():
        again = cx.solve_raw(_opts())
        assert again[0] == 0 and again[3] == want[3] and _bits(again[1]) == _bits(want[1]) and _bits(again[2]) == _bits(want[2])

    for bad in (np.nan, -np.inf):
        ub = u.copy(); ub[1] = bad
        assert up(cx._h, ub) == _capi.ERR_BAD_ARGUMENT
        unchanged()
    assert L.lpipm_upload_bounded(cx._h, nx, 0, None, nx, None, 0, None, nx, None, dp(c), 0.0, dp(u)) == _capi.UNCONSTRAINED
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
    assert up(split._h, u) == _capi.ERR_UNSUPPORTED
    assert split.resident_bytes() == 0 and coll.calls == 0
    split.close()
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_REFINE", "2")
    refining = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_REFINE")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    assert up(refining._h, u) == _capi.ERR_UNSUPPORTED
    assert refining.resident_bytes() == 0
    refining.close()
    # the bounded entries refuse any other upload
    other = lp_amd.Context(0)
    other.upload(_problem(A_ub, b_ub, A_eq, b_eq, c))
    assert L.lpipm_k_bounded_normal(other._h, dp(np.ones(n)), dp(np.empty((m, m)))) == _capi.ERR_UNSUPPORTED
    other.close()


# ---- 13. nothing of the form leaks -----------------------------------------------------------------------------------------------
def test_an_ordinary_upload_after_a_bounded_solve_is_a_fresh_one(built):
    import lp_amd
    lp = planted_box(*SHAPES[2])
    plain = _problem(*lp[:5])
    cx = lp_amd.Context(0)
    cx.upload(_problem(*lp[:6]))
    assert cx.solve_raw(_opts())[0] == 0
    cx.upload(plain)
    after = cx.solve_raw(_opts())
    cx.close()
    fresh = lp_amd.Context(0)
    fresh.upload(plain)
    want = fresh.solve_raw(_opts())
    fresh.close()
    assert after[0] == want[0] and after[3] == want[3]
    assert _bits(after[1]) == _bits(want[1]) and _bits(after[2]) == _bits(want[2])
