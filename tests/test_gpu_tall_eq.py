"""The tall form with equality rows (lpipm_upload_ub_eq_tall): K = X^T W_s X + E_x on the `ub` rows, the `eq` rows
through the Schur complement S = A_eq K^-1 A_eq^T on K's factor, the solve on K split into its halves around the correction.
Whole solves against the oracle (as generated and with permuted columns) and against lpipm_upload_ub_eq, the other exits, a
large-m shape against its planted optimum, the kernel entries against numpy / the oracle's dense sym_solve, m_eq = 0, scaling,
memory, phase times and the refusals.  Generator, shapes and the host-side conditions on them: tests/test_tall_eq_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_tall_eq_host import (FACE_CASE, GPU_SHAPES, OPTION_SHAPE, X_TOL, make_tall_eq_solver, permuted, planted_eq, planted_face,
                               slack_form)

pytestmark = pytest.mark.gpu

IDS = [f"{m}x{nx}+{me}" for _, m, nx, me in GPU_SHAPES]
OPTION_KW = [(("ip", 0),), (("tol", 1e-6),), (("max_iter", 3),)]
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def _problem(X, b, Ae, be, c):
    import lp_amd
    p = lp_amd.Problem.target(c).ub(X, b)
    return (p.eq(Ae, be) if Ae.shape[0] else p).build()


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _oracle_pair(case, kw=()):
    """The C oracle on the slack form of the case as generated and with its structural columns permuted (x mapped back):
    computed once, shared, never written to."""
    from oracle import capi as oracle
    seed, m, nx, me = case
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    ref = oracle.solve(*slack_form(X, b, Ae, be, c), opts=oracle.default_opts(**dict(kw)), want_log=False)
    Xp, Aep, cp, perm = permuted(X, Ae, c, seed)
    alt = oracle.solve(*slack_form(Xp, b, Aep, be, cp), opts=oracle.default_opts(**dict(kw)), want_log=False)
    if alt["x_slack"] is not None:
        back = alt["x_slack"].copy()
        back[perm] = alt["x_slack"][:nx]
        alt["x_slack"] = back
    for r in (ref, alt):
        if r["x_slack"] is not None:
            r["x_slack"].setflags(write=False)
    return ref, alt


def _check_against(pair, got, what):
    """Status as the oracle's, an iteration count the oracle produced, x inside the oracle's envelope widened by X_TOL, fun."""
    ref, alt = pair
    rc, x, fun, it, _ = got
    assert ref["status"] == alt["status"]
    assert rc == ref["status"], (what, rc, ref["status"])
    assert it in (ref["iterations"], alt["iterations"]), (what, it, ref["iterations"], alt["iterations"])
    if ref["x_slack"] is not None:
        lo, hi = np.minimum(ref["x_slack"], alt["x_slack"]), np.maximum(ref["x_slack"], alt["x_slack"])
        out = np.maximum(np.maximum(lo - x, x - hi), 0.0).max()
        print(f"\n[measure] {what}: status {rc}, {it} iterations, outside the oracle's envelope {out:.3g} "
              f"(its width {np.abs(hi - lo).max():.3g}), fun rel {abs(fun - ref['fun']) / max(1.0, abs(ref['fun'])):.3g}")
        assert out <= X_TOL, (what, out)
        assert abs(fun - ref["fun"]) <= 1e-6 * max(1.0, abs(ref["fun"])), (what, fun, ref["fun"])


# ---- 1. whole solves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GPU_SHAPES, ids=IDS)
def test_solve_matches_the_oracle_and_upload_ub_eq(ctx, case):
    seed, m, nx, me = case
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    prob = _problem(X, b, Ae, be, c)
    ctx.upload_tall_eq(prob)
    assert (ctx.m, ctx.n) == (m + me, nx + m)
    new = ctx.solve_raw(_opts())
    pair = _oracle_pair(case)
    assert pair[0]["status"] == 0
    _check_against(pair, new, f"tall_eq {m}x{nx}+{me}")
    ctx.upload(prob)                                         # lpipm_upload_ub_eq on the same context
    old = ctx.solve_raw(_opts())
    assert old[0] == 0 and new[0] == old[0] and new[3] == old[3], (old[0], new[0], old[3], new[3])
    err = np.abs(new[1] - old[1]).max()
    print(f"\n[measure] tall_eq vs ub_eq {m}x{nx}+{me}: {new[3]} iterations, max|dx| {err:.3g}")
    assert err <= X_TOL, err
    assert abs(new[2] - old[2]) <= 1e-6 * max(1.0, abs(old[2]))


@pytest.mark.parametrize("kw", OPTION_KW, ids=["ip0", "tol1e-6", "max_iter3"])
def test_solve_options(ctx, kw):
    seed, m, nx, me = OPTION_SHAPE
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    prob = _problem(X, b, Ae, be, c)
    ctx.upload_tall_eq(prob)
    got = ctx.solve_raw(_opts(**dict(kw)))
    pair = _oracle_pair(OPTION_SHAPE, kw)
    if dict(kw).get("max_iter") == 3:
        assert got[0] == 7 and pair[0]["status"] == 7            # IterationLimit, x filled
        assert not np.isnan(got[1]).any()
    else:
        assert pair[0]["status"] == 0
    _check_against(pair, got, f"tall_eq {m}x{nx}+{me} {kw}")
    ctx.upload(prob)
    old = ctx.solve_raw(_opts(**dict(kw)))
    assert got[0] == old[0] and got[3] == old[3]
    assert np.abs(got[1] - old[1]).max() <= X_TOL


# ---- 2. the other exits ---------------------------------------------------------------------------------------------------------
def _infeasible():
    X, b, Ae, be, c, _ = planted_eq(1, 40, 8, 2)
    return X, b, np.vstack([Ae, np.ones((1, 8))]), np.concatenate([be, [-1.0]]), c      # sum x = -1 with x >= 0


def _unbounded():
    X = np.array([[1.0, -1.0, 0.0], [-1.0, 0.5, 0.0], [0.0, -1.0, 0.0]])
    return X, np.ones(3), np.array([[0.0, 1.0, -1.0]]), np.zeros(1), np.array([-1.0, 0.0, 0.0])


@pytest.mark.parametrize("make,status", [(_infeasible, 5), (_unbounded, 6)], ids=["infeasible", "unbounded"])
def test_other_exits(ctx, make, status):
    from oracle import capi as oracle
    X, b, Ae, be, c = make()
    ref = oracle.solve(*slack_form(X, b, Ae, be, c), want_log=False)
    assert ref["status"] == status
    ctx.upload_tall_eq(_problem(X, b, Ae, be, c))
    rc, x, fun, it, _ = ctx.solve_raw(_opts())
    assert rc == status and it == ref["iterations"], (rc, it, ref["iterations"])


def _duplicated_row():
    X, b, Ae, be, c, _ = planted_eq(1, 300, 40, 5)
    return X, b, np.vstack([Ae, Ae[:1]]), np.concatenate([be, be[:1]]), c


def _more_rows_than_columns():
    X, b, Ae, be, c, xs = planted_eq(1, 300, 40, 40)
    row = np.random.default_rng(5).standard_normal((1, 40))
    return X, b, np.vstack([Ae, row]), np.concatenate([be, row @ xs]), c


@pytest.mark.parametrize("make", [_duplicated_row, _more_rows_than_columns], ids=["duplicated_row", "m_eq=nx+1"])
def test_dependent_equality_rows_are_a_numerical_problem(ctx, make):
    """Status only: the failing pivot of S comes at an iteration that depends on rounding."""
    from oracle import capi as oracle
    X, b, Ae, be, c = make()
    assert oracle.solve(*slack_form(X, b, Ae, be, c), want_log=False)["status"] == 2
    ctx.upload_tall_eq(_problem(X, b, Ae, be, c))
    assert ctx.solve_raw(_opts())[0] == 2
    # the context is whole afterwards
    case = GPU_SHAPES[0]
    ctx.upload_tall_eq(_problem(*planted_eq(*case)[:5]))
    assert ctx.solve_raw(_opts())[0] == 0


# ---- 3. many rows, against the planted optimum ---------------------------------------------------------------------------------------
def test_4096_rows_against_the_planted_optimum(built):
    """A shape on which the oracle itself fails (its m x m Cholesky, in its last iteration: asserted on the host in
    tests/test_tall_eq_host.py), so no parity case: Ok, and the planted optimal value (the optimal x is not unique there)."""
    import lp_amd
    seed, m, nx, me = FACE_CASE
    X, b, Ae, be, c, xs = planted_face(seed, m, nx, me)
    cx = lp_amd.Context(0)
    cx.upload_tall_eq(_problem(X, b, Ae, be, c))
    rc, x, fun, it, _ = cx.solve_raw(_opts())
    cx.close()
    fstar = float(c @ xs)
    viol = max(np.maximum(X @ x[:nx] - b, 0.0).max(), np.abs(Ae @ x[:nx] - be).max(), np.maximum(-x, 0.0).max())
    print(f"\n[measure] 4096x32+8: status {rc}, {it} iterations, |fun - f*| {abs(fun - fstar):.3g}, violation {viol:.3g}")
    assert rc == 0
    assert abs(fun - fstar) <= 1e-6 * max(1.0, abs(fstar))
    assert viol <= 1e-6


# ---- 4. the kernel entries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,m", [(40, 300), (600, 700)], ids=["nx40", "nx600"])
@pytest.mark.parametrize("me", [1, 16, 17, 130])
def test_k_tall_schur(ctx, nx, m, me):
    """Zt = A_eq L^-T at the strip tail (1, 16, 17 rows of 16) and at one and two 128-blocks of rows, over one and five
    128-blocks of L (two super-blocks at nx = 600).  S as built: at m_eq > nx it is singular and still A_eq K^-1 A_eq^T.
    Bound: the factor of K + dK with |dK| <= c nx eps |K| gives |dS| <= c nx eps cond(K) |S| (Higham, Accuracy and Stability,
    10.1-10.3); c = 8 covers the two triangular solves and the product; numpy's reference carries the same error."""
    rng = np.random.default_rng(100 * me + nx)
    X, b, Ae, be, c, _ = planted_eq(3, m, nx, me)
    ctx.upload_tall_eq(_problem(X, b, Ae, be, c))
    dinv = np.exp(rng.uniform(-1, 1, nx + m))
    S = ctx.k_tall_schur(dinv)
    K = X.T @ ((1.0 / dinv[nx:])[:, None] * X) + np.diag(1.0 / dinv[:nx])
    ref = Ae @ np.linalg.solve(K, Ae.T)
    il = np.tril_indices(me)
    err = np.abs(S[il] - ref[il]).max()
    bound = 8 * nx * np.finfo(float).eps * np.linalg.cond(K) * np.linalg.norm(ref, 2)
    print(f"\n[measure] S {m}x{nx}+{me}: err {err:.3g}, bound {bound:.3g}, max|S| {np.abs(ref).max():.3g}")
    assert err <= bound, (err, bound)
    Kd = ctx.k_tall_normal(dinv)                             # K on the new upload: from the `ub` rows
    ik = np.tril_indices(nx)
    assert np.abs(Kd[ik] - K[ik]).max() <= 1e-13 * np.sqrt(m) * np.abs(K).max()


def _iterate(rng, m, n, spread):                       # tests/test_gpu_tall_form.py::_iterate
    x = np.exp(rng.uniform(-spread, spread, n)); z = np.exp(rng.uniform(-spread, spread, n))
    return x, rng.standard_normal(m), z, float(np.exp(rng.uniform(-1, 1))), float(np.exp(rng.uniform(-1, 1)))


@pytest.mark.parametrize("spread", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("seed,shape", [(2, (129, 17, 3)), (5, (520, 130, 9))], ids=["129x17+3", "520x130+9"])
def test_k_tall_sym_solve(ctx, seed, shape, spread):
    """Against the oracle's dense sym_solve.  The bound is tests/test_gpu_tall_form.py's 1e-8 where the numpy emulation of the
    algebra meets it with a factor 10 to spare on these iterates, else 10 x the emulation's own error (measured: at most
    4.7e-11, so 1e-8)."""
    from oracle import oracle_np
    m, nx, me = shape
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    A, bs, cs = slack_form(X, b, Ae, be, c)
    n, mm = nx + m, m + me
    ctx.upload_tall_eq(_problem(X, b, Ae, be, c))
    rng = np.random.default_rng(int(10 * spread) + seed)
    x, _, z, _, _ = _iterate(rng, mm, n, spread)
    timing = {"adat": 0.0, "chol": 0.0, "solves": 0.0, "gemv": 0.0}
    eq = oracle_np._EqSolver(A, x, z, 0, timing)
    emu = make_tall_eq_solver(nx, m)(A, x, z, 0, timing)
    assert eq.ok and emu.ok
    pairs = [(cs, bs), (rng.standard_normal(n), rng.standard_normal(mm))]          # (c, b) and a general (r1, r2)
    refs = [eq.sym_solve(A, r1, r2) for r1, r2 in pairs]
    rel = lambda got, ref: np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    emu_err = max(max(rel(u, ru), rel(v, rv)) for (u, v), (ru, rv) in zip([emu.sym_solve(A, *p) for p in pairs], refs))
    bound = 1e-8 if emu_err <= 1e-9 else 10 * emu_err
    U, V, info = ctx.k_tall_sym_solve(x / z, np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    assert info == 0
    for q, (u, v) in enumerate(refs):
        print(f"\n[measure] sym_solve {m}x{nx}+{me} spread {spread} rhs {q}: u {rel(U[q], u):.3g} v {rel(V[q], v):.3g} "
              f"(emulation {emu_err:.3g}, bound {bound:.3g})")
        assert rel(U[q], u) <= bound and rel(V[q], v) <= bound, (q, rel(U[q], u), rel(V[q], v))
    U1, V1, info = ctx.k_tall_sym_solve(x / z, pairs[1][0], pairs[1][1])          # the corrector's shape
    assert info == 0
    assert rel(U1[0], refs[1][0]) <= bound and rel(V1[0], refs[1][1]) <= bound


def _compare(dev, ref):                                 # tests/test_gpu_tall_form.py::_compare
    assert ref["status"] == 0 and dev["info"] == 0
    scale = lambda a: max(1.0, np.abs(a).max())
    for k in ("d_x", "d_y", "d_z", "x", "y", "z"):
        assert np.abs(dev[k] - ref[k]).max() <= 1e-8 * scale(ref[k]), k
    for k in ("d_tau", "d_kappa", "tau", "kappa"):
        assert abs(dev[k] - ref[k]) <= 1e-8 * max(1.0, abs(ref[k])), k
    assert abs(dev["alpha"] - ref["alpha"]) <= 1e-8


@pytest.mark.parametrize("ip", [False, True])
def test_one_iteration_on_the_new_upload(ctx, ip):
    """One loop body (lpipm_k_iteration) against oracle.iteration from arbitrary iterates: head, Schur build, both sym_solves,
    step, on the bounds tests/test_gpu_tall_form.py has for the pure-`ub` form (its shape 333 x 100, spread 2, plus 7 rows)."""
    from oracle import capi as oracle
    seed, m, nx, me = 11, 333, 100, 7
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    A, bs, cs = slack_form(X, b, Ae, be, c)
    ctx.upload_tall_eq(_problem(X, b, Ae, be, c))
    rng = np.random.default_rng(100 * seed + int(ip))
    for trial in range(3):
        x, y, z, tau, kappa = _iterate(rng, m + me, nx + m, 2.0)
        ref = oracle.iteration(A, bs, cs, x, y, z, tau, kappa, ip=ip)
        _compare(ctx.k_iteration(_opts(), x, y, z, tau, kappa, ip=ip), ref)


# ---- 5. m_eq = 0 is lpipm_upload_ub_tall ---------------------------------------------------------------------------------------------
def test_without_eq_rows_it_is_the_tall_upload(built):
    import lp_amd
    m, nx = 300, 33
    X, b, _, _, c, _ = planted_eq(4, m, nx, 0)
    prob = lp_amd.Problem.target(c).ub(X, b).build()
    a, t = lp_amd.Context(0), lp_amd.Context(0)
    a.upload_tall_eq(prob)
    t.upload(prob, tall=True)
    assert (a.m, a.n) == (t.m, t.n) and a.resident_bytes() == t.resident_bytes()
    ra, rt = a.solve_raw(_opts()), t.solve_raw(_opts())
    a.close(); t.close()
    assert ra[0] == 0 and ra[0] == rt[0] and ra[3] == rt[3]
    assert _bits(ra[1]) == _bits(rt[1]) and _bits(ra[2]) == _bits(rt[2])


# ---- 6. scaling -------------------------------------------------------------------------------------------------------------------
def test_scaling_is_the_host_scaled_solve(built):
    import lp_amd
    seed, m, nx, me = OPTION_SHAPE
    X, b, Ae, be, c, xs = planted_eq(seed, m, nx, me)
    rng = np.random.default_rng(44)
    er, ec = rng.integers(-8, 9, m + me).astype(np.int32), rng.integers(-8, 9, nx).astype(np.int32)
    sc = lambda M, r, cexp: np.ldexp(M, r[:, None] + cexp[None, :])
    Xd, Aed, bd, bed, cd = sc(X, er[:m], ec), sc(Ae, er[m:], ec), np.ldexp(b, er[:m]), np.ldexp(be, er[m:]), np.ldexp(c, ec)
    o = _opts()
    cx = lp_amd.Context(0).set_scaling(8)
    cx.upload_tall_eq(_problem(Xd, bd, Aed, bed, cd))          # optimum: ldexp(x*, -ec)
    kr, kc = cx.scaling()
    assert kr.shape == (m + me,) and kc.shape == (nx + m,) and np.array_equal(kc[nx:], -kr[:m])
    assert np.any(kr[:m] != 0) and np.any(kr[m:] != 0) and np.any(kc[:nx] != 0)
    got = cx.solve_raw(o, want_log=True)
    cx.close()
    ref_cx = lp_amd.Context(0)
    ref_cx.upload_tall_eq(_problem(sc(Xd, kr[:m], kc[:nx]), np.ldexp(bd, kr[:m]), sc(Aed, kr[m:], kc[:nx]), np.ldexp(bed, kr[m:]),
                                   np.ldexp(cd, kc[:nx])))
    ref = ref_cx.solve_raw(o, want_log=True)
    ref_cx.close()
    # tests/test_gpu_scaling.py's criterion: status, count, every log row and fun bit for bit, x = ldexp(x_ref, kc) bit for bit
    assert got[0] == 0 and got[0] == ref[0] and got[3] == ref[3]
    assert _bits(got[1]) == _bits(np.ldexp(ref[1], kc))
    assert _bits(got[2]) == _bits(ref[2])
    assert len(got[4]) == len(ref[4]) and _bits(np.array(got[4])) == _bits(np.array(ref[4]))
    assert np.abs(np.ldexp(got[1][:nx], ec) - xs).max() <= X_TOL          # x is in the caller's units


# ---- 7. memory, phase times --------------------------------------------------------------------------------------------------------
def test_resident_bytes_grow_linearly_in_m_ub(built):
    import lp_amd
    nx, me, sizes = 64, 8, {}
    for m in (1024, 2048, 4096):
        X, b, Ae, be, c, _ = planted_eq(20, m, nx, me)
        cx = lp_amd.Context(0)
        cx.upload_tall_eq(_problem(X, b, Ae, be, c))
        sizes[m] = cx.resident_bytes()
        cx.close()
    print(f"\n[measure] resident bytes, nx = 64, m_eq = 8: {sizes}")
    # tests/test_gpu_tall_form.py's criterion at each doubling: linear growth gives at most 2, quadratic growth gives 4 (the
    # chunk slabs of the launch that builds K grow in steps with the contraction length, hence not a fixed increment)
    assert sizes[1024] < sizes[2048] <= 2.5 * sizes[1024], sizes
    assert sizes[2048] < sizes[4096] <= 2.5 * sizes[2048], sizes
    assert sizes[4096] < 64 << 20, sizes                      # M alone would be 135 MB


def test_phase_times(built):
    import lp_amd
    case = GPU_SHAPES[1]
    cx = lp_amd.Context(0)
    cx.upload_tall_eq(_problem(*planted_eq(*case)[:5]))
    plain = cx.solve_raw(_opts())
    cx.set_profiling(1)
    rc, x, fun, it, _ = cx.solve_raw(_opts())
    t = cx.phase_times()
    cx.close()
    assert rc == 0 and it == plain[3] and _bits(x) == _bits(plain[1])
    assert t["adat_launches"] == it and t["iterations"] == it          # the build of K only: S's launch is not counted
    assert t["adat_ms"] > 0 and t["potrf_ms"] > 0 and t["trsv_ms"] > 0


def test_python_context_tracks_the_eq_rows_across_uploads(built):
    """Context.k_tall_normal / k_tall_schur size their outputs from the resident problem's `eq` rows: every upload that succeeds
    sets the count (a device upload too), and a rejected upload leaves the resident problem's count alone."""
    import lp_amd
    import torch
    seed, m, nx, me = 1, 40, 8, 2
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    dinv = np.exp(np.random.default_rng(8).uniform(-1, 1, nx + m))
    K = X.T @ ((1.0 / dinv[nx:])[:, None] * X) + np.diag(1.0 / dinv[:nx])
    il = np.tril_indices(nx)
    cx = lp_amd.Context(0)
    cx.upload_tall_eq(_problem(X, b, Ae, be, c))
    with pytest.raises(ValueError):
        cx.upload(_problem(X, b, Ae, be, c), tall=True)          # rejected before the library is called
    assert cx.k_tall_schur(dinv).shape == (me, me)
    Kd = cx.k_tall_normal(dinv)
    assert Kd.shape == (nx, nx) and np.abs(Kd[il] - K[il]).max() <= 1e-13 * np.sqrt(m) * np.abs(K).max()
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda:0")
    cx.upload_device(dev(X), dev(b), dev(c), form="ub_tall")     # the same X without its `eq` rows
    assert (cx.m, cx.n) == (m, nx + m)
    Kd = cx.k_tall_normal(dinv)
    assert Kd.shape == (nx, nx) and np.abs(Kd[il] - K[il]).max() <= 1e-13 * np.sqrt(m) * np.abs(K).max()
    cx.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
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
    from lp_amd import _capi, synth
    L = _capi.lib()
    seed, m, nx, me = 1, 40, 8, 2
    X, b, Ae, be, c, _ = planted_eq(seed, m, nx, me)
    X, Ae = np.ascontiguousarray(X), np.ascontiguousarray(Ae)
    cx = lp_amd.Context(0)
    with pytest.raises(ValueError):
        cx.upload_tall_eq(lp_amd.Problem.target(c).eq(Ae, be).build())
    with pytest.raises(ValueError):
        cx.upload(_problem(X, b, Ae, be, c), tall=True)          # tall=True keeps refusing `eq` rows
    cx.upload_tall_eq(_problem(X, b, Ae, be, c))
    want = cx.solve_raw(_opts())
    assert want[0] == 0

    def same_bits():
        got = cx.solve_raw(_opts())
        assert got[0] == want[0] and got[3] == want[3] and _bits(got[1]) == _bits(want[1]) and _bits(got[2]) == _bits(want[2])

    up = lambda *a: (lambda: L.lpipm_upload_ub_eq_tall(cx._h, *a))
    refused = [
        (up(nx, 0, None, nx, None, 0, None, nx, None, dp(c), 0.0), _capi.UNCONSTRAINED),
        (up(nx, 0, None, nx, None, me, dp(Ae), nx, dp(be), dp(c), 0.0), _capi.ERR_UNSUPPORTED),       # no `ub` row: not a tall LP
        (up(nx, m, None, nx, dp(b), me, dp(Ae), nx, dp(be), dp(c), 0.0), _capi.ERR_BAD_ARGUMENT),
        (up(nx, m, dp(X), nx, None, me, dp(Ae), nx, dp(be), dp(c), 0.0), _capi.ERR_BAD_ARGUMENT),
        (up(nx, m, dp(X), nx, dp(b), me, None, nx, dp(be), dp(c), 0.0), _capi.ERR_BAD_ARGUMENT),
        (up(nx, m, dp(X), nx, dp(b), me, dp(Ae), nx, None, dp(c), 0.0), _capi.ERR_BAD_ARGUMENT),
        (up(nx, m, dp(X), nx, dp(b), me, dp(Ae), nx, dp(be), None, 0.0), _capi.ERR_BAD_ARGUMENT),
        (up(nx, m, dp(X), nx - 1, dp(b), me, dp(Ae), nx, dp(be), dp(c), 0.0), _capi.ERR_BAD_ARGUMENT),
        (up(nx, m, dp(X), nx, dp(b), me, dp(Ae), nx - 1, dp(be), dp(c), 0.0), _capi.ERR_BAD_ARGUMENT),
    ]
    import torch
    bs, cs = np.ones(m + me), np.ones(nx + m)
    bd, cd = torch.ones(m + me, dtype=torch.float64, device="cuda:0"), torch.ones(nx + m, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize(0)
    unsupported = lambda call: (call, _capi.ERR_UNSUPPORTED)
    refused += [
        unsupported(lambda: cx.solve_raw(_opts(solver_type=1))[0]),
        unsupported(lambda: cx.solve_raw(_opts(solver_type=2))[0]),
        unsupported(lambda: L.lpipm_update_vectors(cx._h, dp(bs), dp(cs))),
        unsupported(lambda: L.lpipm_update_vectors_device(cx._h, C.c_void_p(bd.data_ptr()), C.c_void_p(cd.data_ptr()))),
        unsupported(lambda: L.lpipm_k_adat(cx._h, dp(np.ones(nx + m)), dp(np.empty((m + me, m + me))), 1, None)),
    ]
    for k, (call, code) in enumerate(refused):           # after EACH refused call the resident problem solves to the same bits
        rc = call()
        assert rc == code, (k, rc, code)
        same_bits()
    # lpipm_k_tall_schur on any other upload
    cx.upload(_problem(X, b, Ae[:0], be[:0], c), tall=True)
    assert L.lpipm_k_tall_schur(cx._h, dp(np.ones(nx + m)), dp(np.empty((me, me)))) == _capi.ERR_UNSUPPORTED
    cx.upload(_problem(X, b, Ae, be, c))
    assert L.lpipm_k_tall_schur(cx._h, dp(np.ones(nx + m)), dp(np.empty((me, me)))) == _capi.ERR_UNSUPPORTED
    # an ordinary upload afterwards on the same context solves as on a fresh one
    cx.upload_tall_eq(_problem(X, b, Ae, be, c))
    same_bits()
    A, b2, c2, _ = synth.planted_lp(3, 64, 160)
    cx.upload_arrays(A, b2, c2)
    after = cx.solve_raw(_opts())
    cx.close()
    fresh = lp_amd.Context(0)
    fresh.upload_arrays(A, b2, c2)
    ordinary = fresh.solve_raw(_opts())
    fresh.close()
    assert after[0] == 0 and after[0] == ordinary[0] and after[3] == ordinary[3]
    assert _bits(after[1]) == _bits(ordinary[1]) and _bits(after[2]) == _bits(ordinary[2])
    # a column-split context and one with the refined solves
    split = lp_amd.Context(0)
    coll = _NeverCalled()
    split.set_collective(1, 2, coll)
    assert L.lpipm_upload_ub_eq_tall(split._h, nx, m, dp(X), nx, dp(b), me, dp(Ae), nx, dp(be), dp(c), 0.0) == _capi.ERR_UNSUPPORTED
    assert split.resident_bytes() == 0 and coll.calls == 0
    split.close()
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_REFINE", "2")
    refining = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_REFINE")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    assert L.lpipm_upload_ub_eq_tall(refining._h, nx, m, dp(X), nx, dp(b), me, dp(Ae), nx, dp(be), dp(c), 0.0) == _capi.ERR_UNSUPPORTED
    assert refining.resident_bytes() == 0
    refining.close()
