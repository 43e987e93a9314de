"""The tall inequality form (lpipm_upload_ub_tall): a pure-`ub` LP whose solves factor the nx x nx reduced system
K = X^T W_s X + E_x instead of the m x m normal matrix.  Whole solves against the oracle on the host-assembled slack form and
against the existing structural-slack path, the two kernel entries against numpy / the oracle's dense sym_solve, one loop
body against oracle.iteration, the arena's growth with m, a size the slack form cannot reasonably serve, the equilibration's
bit-identity criterion and the refusals."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-6


def planted(seed, m, nx):
    """A planted nondegenerate vertex of min c^T x, X x <= b, x >= 0: k = nx // 2 basic structural variables and k active rows.
    -> X, b, c, x*"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    k = nx // 2
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:k]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, k)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    c = -X.T @ lam + mu
    return X, b, c, xs


def slack_form(X, b, c):
    m, nx = X.shape
    return np.hstack([X, np.eye(m)]), b, np.concatenate([c, np.zeros(m)])


def _problem(X, b, c):
    import lp_amd
    return lp_amd.Problem.target(c).ub(X, b).build()


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _oracle_opts(**kw):
    from oracle import capi as oracle
    return oracle.default_opts(**kw)


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def _oracle_solve(seed, m, nx, kw=()):
    """The oracle on the slack form of planted(seed, m, nx): computed once, shared, never written to."""
    from oracle import capi as oracle
    A, b, c = slack_form(*planted(seed, m, nx)[:3])
    ref = oracle.solve(A, b, c, opts=_oracle_opts(**dict(kw)), want_log=False)
    if ref["x_slack"] is not None:
        ref["x_slack"].setflags(write=False)
    return ref


def _check_against(ref, got, what):
    rc, x, fun, it, _ = got
    assert rc == ref["status"], (what, rc, ref["status"])
    assert it == ref["iterations"], (what, it, ref["iterations"])
    if ref["x_slack"] is not None:
        err = np.abs(x - ref["x_slack"]).max()
        print(f"\n[measure] {what}: status {rc}, {it} iterations, max|x - x_oracle| {err:.3g}, "
              f"fun rel {abs(fun - ref['fun']) / max(1.0, abs(ref['fun'])):.3g}")
        assert err <= X_TOL, (what, err)
        assert abs(fun - ref["fun"]) <= 1e-6 * max(1.0, abs(ref["fun"])), (what, fun, ref["fun"])


# ---- 1. solves against the oracle ----------------------------------------------------------------------------------------------
SHAPES = [(3, 2), (40, 7), (129, 17), (130, 129), (300, 33), (520, 130), (700, 257), (1100, 513), (1500, 16), (2000, 100)]


@pytest.mark.parametrize("seed,shape", list(enumerate(SHAPES)), ids=[f"{m}x{nx}" for m, nx in SHAPES])
def test_solve_matches_the_oracle(ctx, seed, shape):
    m, nx = shape
    X, b, c, _ = planted(seed, m, nx)
    ctx.upload(_problem(X, b, c), tall=True)
    assert (ctx.m, ctx.n) == (m, nx + m)
    got = ctx.solve_raw(_opts())
    ref = _oracle_solve(seed, m, nx)
    assert ref["status"] == 0
    _check_against(ref, got, f"tall {m}x{nx}")


@pytest.mark.parametrize("seed,shape", [(2, (129, 17)), (5, (520, 130))], ids=["129x17", "520x130"])
@pytest.mark.parametrize("kw", [(("ip", 0),), (("tol", 1e-6),), (("max_iter", 3),)], ids=["ip0", "tol1e-6", "max_iter3"])
def test_solve_options(ctx, seed, shape, kw):
    m, nx = shape
    X, b, c, _ = planted(seed, m, nx)
    ctx.upload(_problem(X, b, c), tall=True)
    got = ctx.solve_raw(_opts(**dict(kw)))
    ref = _oracle_solve(seed, m, nx, kw)
    if dict(kw).get("max_iter") == 3:
        assert got[0] == 7 and ref["status"] == 7            # IterationLimit, x filled
        assert not np.isnan(got[1]).any()
    else:
        assert ref["status"] == 0
    _check_against(ref, got, f"tall {m}x{nx} {kw}")


@pytest.mark.parametrize("X,b,c,status", [
    ([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]], [-1.0, 2.0, 2.0], [1.0, 1.0], 5),        # Infeasible
    ([[1.0, -1.0], [-1.0, 0.5], [0.0, -1.0]], [1.0, 1.0, 1.0], [-1.0, 0.0], 6),     # Unbounded
], ids=["infeasible", "unbounded"])
def test_other_exits(ctx, X, b, c, status):
    from oracle import capi as oracle
    X, b, c = np.array(X), np.array(b), np.array(c)
    ref = oracle.solve(*slack_form(X, b, c), want_log=False)
    assert ref["status"] == status
    ctx.upload(_problem(X, b, c), tall=True)
    rc, x, fun, it, _ = ctx.solve_raw(_opts())
    assert rc == status and it == ref["iterations"], (rc, it, ref["iterations"])


# ---- 2. tall against the existing structural-slack path ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape", [(1, (40, 7)), (2, (129, 17)), (5, (520, 130)), (6, (700, 257))],
                         ids=["40x7", "129x17", "520x130", "700x257"])
def test_tall_agrees_with_upload_ub_eq(ctx, seed, shape):
    m, nx = shape
    X, b, c, _ = planted(seed, m, nx)
    prob = _problem(X, b, c)
    o = _opts()
    ctx.upload(prob)
    old = ctx.solve_raw(o)
    ctx.upload(prob, tall=True)
    new = ctx.solve_raw(o)
    assert old[0] == 0 and new[0] == old[0] and new[3] == old[3], (old[0], new[0], old[3], new[3])
    err = np.abs(new[1] - old[1]).max()
    print(f"\n[measure] tall vs ub_eq {m}x{nx}: {new[3]} iterations, max|dx| {err:.3g}")
    assert err <= X_TOL, err


# ---- 3. K against numpy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape", [(2, (129, 17)), (6, (700, 257)), (9, (2000, 100))], ids=["129x17", "700x257", "2000x100"])
def test_k_tall_normal(ctx, seed, shape):
    m, nx = shape
    X, b, c, _ = planted(seed, m, nx)
    ctx.upload(_problem(X, b, c), tall=True)
    rng = np.random.default_rng(1000 + seed)
    dinv = np.exp(rng.uniform(-3, 3, nx + m))
    K = ctx.k_tall_normal(dinv)
    ref = X.T @ ((1.0 / dinv[nx:])[:, None] * X) + np.diag(1.0 / dinv[:nx])
    il = np.tril_indices(nx)
    err = np.abs(K[il] - ref[il]).max()
    print(f"\n[measure] K {m}x{nx}: err / (sqrt(m) max|K|) {err / (np.sqrt(m) * np.abs(ref).max()):.3g}")
    assert err <= 1e-13 * np.sqrt(m) * np.abs(ref).max(), err          # the A.D.A^T kernel test's bound: contraction length m


# ---- 4. the reduced sym_solve against the oracle's dense one ----------------------------------------------------------------------
def _iterate(rng, m, n, spread):                       # tests/test_gpu_iteration.py::_iterate
    x = np.exp(rng.uniform(-spread, spread, n)); z = np.exp(rng.uniform(-spread, spread, n))
    return x, rng.standard_normal(m), z, float(np.exp(rng.uniform(-1, 1))), float(np.exp(rng.uniform(-1, 1)))


@pytest.mark.parametrize("spread", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("seed,shape", [(2, (129, 17)), (5, (520, 130))], ids=["129x17", "520x130"])
def test_k_tall_sym_solve(ctx, seed, shape, spread):
    from oracle import oracle_np
    m, nx = shape
    X, b, c, _ = planted(seed, m, nx)
    A, bs, cs = slack_form(X, b, c)
    n = nx + m
    ctx.upload(_problem(X, b, c), tall=True)
    rng = np.random.default_rng(int(10 * spread) + seed)
    x, _, z, _, _ = _iterate(rng, m, n, spread)
    timing = {"adat": 0.0, "chol": 0.0, "solves": 0.0, "gemv": 0.0}
    eq = oracle_np._EqSolver(A, x, z, 0, timing)
    assert eq.ok
    pairs = [(cs, bs), (rng.standard_normal(n), rng.standard_normal(m))]          # (c, b) and a general (r1, r2)
    refs = [eq.sym_solve(A, r1, r2) for r1, r2 in pairs]
    rel = lambda got, ref: np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
    U, V, info = ctx.k_tall_sym_solve(x / z, np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]))
    assert info == 0
    for q, (u, v) in enumerate(refs):
        print(f"\n[measure] sym_solve {m}x{nx} spread {spread} rhs {q}: u {rel(U[q], u):.3g} v {rel(V[q], v):.3g}")
        assert rel(U[q], u) <= 1e-8 and rel(V[q], v) <= 1e-8, (q, rel(U[q], u), rel(V[q], v))
    # the corrector's shape: one right-hand side
    U1, V1, info = ctx.k_tall_sym_solve(x / z, pairs[1][0], pairs[1][1])
    assert info == 0
    assert rel(U1[0], refs[1][0]) <= 1e-8 and rel(V1[0], refs[1][1]) <= 1e-8


# ---- 5. one loop body against oracle.iteration ----------------------------------------------------------------------------------------
def _compare(dev, ref, x0, z0):                       # tests/test_gpu_iteration.py::_compare
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


@pytest.mark.parametrize("seed,shape,spread", [(1, (40, 7), 1.0), (11, (333, 100), 2.0), (12, (420, 200), 1.5)],
                         ids=["40x7", "333x100", "420x200"])
@pytest.mark.parametrize("ip", [False, True])
def test_one_iteration_on_a_tall_upload(ctx, seed, shape, spread, ip):
    from oracle import capi as oracle
    m, nx = shape
    X, b, c, _ = planted(seed, m, nx)
    A, bs, cs = slack_form(X, b, c)
    ctx.upload(_problem(X, b, c), tall=True)
    rng = np.random.default_rng(100 * seed + int(ip))
    o = _opts()
    for trial in range(4):
        x, y, z, tau, kappa = _iterate(rng, m, nx + m, spread)
        ref = oracle.iteration(A, bs, cs, x, y, z, tau, kappa, ip=ip)
        dev = ctx.k_iteration(o, x, y, z, tau, kappa, ip=ip)
        _compare(dev, ref, x, z)


def test_passes_over_a_on_a_tall_upload(ctx):
    """lpipm_k_gemv_n / _t / _dual see A = [X I] on a tall upload as on any other."""
    m, nx = 333, 100
    X, b, c, _ = planted(11, m, nx)
    A, _, _ = slack_form(X, b, c)
    ctx.upload(_problem(X, b, c), tall=True)
    rng = np.random.default_rng(3)
    W, V = rng.standard_normal((2, nx + m)), rng.standard_normal((2, m))
    tol = 1e-12 * np.sqrt(nx + m)
    Y, _ = ctx.k_gemv_n(W)
    assert np.abs(Y - W @ A.T).max() <= tol * max(1.0, np.abs(W @ A.T).max())
    U, _ = ctx.k_gemv_t(V)
    assert np.abs(U - V @ A).max() <= tol * max(1.0, np.abs(V @ A).max())
    Aw, ATv, _ = ctx.k_gemv_dual(W[0], V[0])
    assert np.abs(Aw - A @ W[0]).max() <= tol * max(1.0, np.abs(A @ W[0]).max())
    assert np.abs(ATv - A.T @ V[0]).max() <= tol * max(1.0, np.abs(A.T @ V[0]).max())


# ---- 6. memory grows with m nx, not m^2 ---------------------------------------------------------------------------------------------
def test_resident_bytes_grow_linearly_in_m(built):
    import lp_amd
    nx, sizes = 64, {}
    for m in (16384, 32768):
        X, b, c, _ = planted(20, m, nx)
        cx = lp_amd.Context(0)
        cx.upload(_problem(X, b, c), tall=True)
        sizes[m] = cx.resident_bytes()
        cx.close()
    print(f"\n[measure] resident bytes, nx = 64: {sizes}")
    assert sizes[32768] <= 2.5 * sizes[16384], sizes       # linear growth gives 2, quadratic gives 4
    assert sizes[32768] < (1 << 30), sizes                 # M alone would be 8.6 GB


# ---- 7. a size the slack form cannot reasonably serve ---------------------------------------------------------------------------------
def test_8192_rows_against_the_planted_optimum(built):
    import lp_amd
    m, nx = 8192, 64
    X, b, c, xs = planted(21, m, nx)
    cx = lp_amd.Context(0)
    cx.upload(_problem(X, b, c), tall=True)
    rc, x, fun, it, _ = cx.solve_raw(_opts())
    cx.close()
    fstar = float(c @ xs)
    ex, ef, viol = np.abs(x[:nx] - xs).max(), abs(fun - fstar), np.maximum(X @ x[:nx] - b, 0.0).max()
    print(f"\n[measure] 8192x64: status {rc}, {it} iterations, |x - x*| {ex:.3g}, |fun - c.x*| {ef:.3g}, violation {viol:.3g}")
    assert rc == 0
    assert ex <= X_TOL
    assert ef <= 1e-6 * max(1.0, abs(fstar))
    assert viol <= 1e-6


# ---- 8. scaling ---------------------------------------------------------------------------------------------------------------------
def test_scaling_is_the_host_scaled_solve(built):
    import lp_amd
    m, nx = 300, 33
    X, b, c, xs = planted(4, m, nx)
    rng = np.random.default_rng(44)
    er, ec = rng.integers(-8, 9, m).astype(np.int32), rng.integers(-8, 9, nx).astype(np.int32)
    Xd, bd, cd = np.ldexp(X, er[:, None] + ec[None, :]), np.ldexp(b, er), np.ldexp(c, ec)     # optimum: ldexp(x*, -ec)
    o = _opts()
    cx = lp_amd.Context(0).set_scaling(8)
    cx.upload(_problem(Xd, bd, cd), tall=True)
    kr, kc = cx.scaling()
    assert kr.shape == (m,) and kc.shape == (nx + m,) and np.array_equal(kc[nx:], -kr)
    assert np.any(kr != 0) and np.any(kc[:nx] != 0)
    got = cx.solve_raw(o, want_log=True)
    cx.close()
    ref_cx = lp_amd.Context(0)
    ref_cx.upload(_problem(np.ldexp(Xd, kr[:, None] + kc[None, :nx]), np.ldexp(bd, kr), np.ldexp(cd, kc[:nx])), tall=True)
    ref = ref_cx.solve_raw(o, want_log=True)
    ref_cx.close()
    # tests/test_gpu_scaling.py's criterion: status, count, every log row and fun bit for bit, x = ldexp(x_ref, kc) bit for bit
    assert got[0] == 0 and got[0] == ref[0] and got[3] == ref[3]
    assert _bits(got[1]) == _bits(np.ldexp(ref[1], kc))
    assert _bits(got[2]) == _bits(ref[2])
    assert len(got[4]) == len(ref[4]) and _bits(np.array(got[4])) == _bits(np.array(ref[4]))
    # ... and x is in the caller's units
    assert np.abs(np.ldexp(got[1][:nx], ec) - xs).max() <= X_TOL


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(built):
    import lp_amd
    from lp_amd import _capi, synth
    import ctypes as C
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    m, nx = 40, 7
    X, b, c, _ = planted(1, m, nx)
    cx = lp_amd.Context(0)
    with pytest.raises(ValueError):
        cx.upload(lp_amd.Problem.target(c).ub(X, b).eq(np.ones((1, nx)), np.ones(1)).build(), tall=True)
    with pytest.raises(ValueError):
        cx.upload(lp_amd.Problem.target(c).eq(np.ones((1, nx)), np.ones(1)).build(), tall=True)
    cx.upload(_problem(X, b, c), tall=True)
    for st in (1, 2):
        assert cx.solve_raw(_opts(solver_type=st))[0] == _capi.ERR_UNSUPPORTED
    bs, cs = np.ones(m), np.ones(nx + m)
    assert _capi.lib().lpipm_update_vectors(cx._h, dp(bs), dp(cs)) == _capi.ERR_UNSUPPORTED
    d, M = np.ones(nx + m), np.empty((m, m))
    assert _capi.lib().lpipm_k_adat(cx._h, dp(d), dp(M), 1, None) == _capi.ERR_UNSUPPORTED
    assert _capi.lib().lpipm_upload_ub_tall(cx._h, nx, 0, None, nx, None, dp(c), 0.0) == _capi.UNCONSTRAINED
    assert _capi.lib().lpipm_upload_ub_tall(cx._h, nx, m, dp(X), nx - 1, dp(b), dp(c), 0.0) == _capi.ERR_BAD_ARGUMENT
    assert cx.solve_raw(_opts())[0] == 0                     # the refused calls left the tall upload as it was
    # an ordinary upload on the same context afterwards solves as on a fresh one; the tall entries then refuse
    A, b2, c2, _ = synth.planted_lp(3, 64, 160)
    cx.upload_arrays(A, b2, c2)
    after = cx.solve_raw(_opts())
    assert _capi.lib().lpipm_k_tall_normal(cx._h, dp(np.ones(160)), dp(np.empty((160, 160)))) == _capi.ERR_UNSUPPORTED
    cx.close()
    fresh = lp_amd.Context(0)
    fresh.upload_arrays(A, b2, c2)
    want = fresh.solve_raw(_opts())
    fresh.close()
    assert after[0] == 0 and after[0] == want[0] and after[3] == want[3]
    assert _bits(after[1]) == _bits(want[1]) and _bits(after[2]) == _bits(want[2])
