"""Dual values and reduced costs of the last solve (lpipm_get_duals), without a device: the oracle's duals, built
by looping the oracle's own loop body from the blind start and proved by that loop's x / tau; the three identities that tie
y, z, tau, kappa to the logged indicators; how far the oracle's duals move under a column permutation (the condition the GPU
parity inputs must meet); Problem.denormalize_duals; the new symbols.

The inputs, the oracle construction and the identity checks of tests/test_gpu_duals.py live here."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from lp_amd._capi import DualInfo            # (lpipm_dual_info: without the getter's ABI nothing in this file has a subject)
from test_tall_eq_host import permuted, planted_eq, slack_form

X_TOL = 1e-6
EPS = 2.0 ** -53                      # unit roundoff of fp64

PLANTED = [(24, 56), (48, 96), (130, 300)]                      # lpipm_upload: m no multiple of 128, n no multiple of 16
PLANTED_SEED = 3
PLANTED_EQ = [(1, 40, 8, 2), (1, 300, 40, 5), (1, 300, 40, 39)]  # lpipm_upload_ub_eq / _slack: (seed, m_ub, nx, m_eq)
CASES = [("planted",) + s for s in PLANTED] + [("eq",) + s for s in PLANTED_EQ]
IDS = [f"planted{m}x{n}" for m, n in PLANTED] + [f"eq{m}x{nx}+{me}" for _, m, nx, me in PLANTED_EQ]


# planted_eq with its `eq` rows dropped (m_eq = 0): the inputs of lpipm_upload_slack in the GPU parity test
EQ_DROPPED = [(1, 40, 8, 0), (1, 300, 40, 0)]
ALL_CASES = CASES + [("eq",) + s for s in EQ_DROPPED]
ALL_IDS = IDS + [f"eq{m}x{nx}+{me}" for _, m, nx, me in EQ_DROPPED]

# the members of the bit-identity batches of tests/test_gpu_duals.py: 24 x 56 in the dense forms; 24 `ub` + 8 `eq` rows over 32
# columns (a 32 x 56 slack form) in the slack forms; 56 `ub` rows (+ 3 `eq` rows) over 24 columns in the tall forms
MEMBER_SEED = 11
SLACK_MEMBER = (24, 32, 8)            # (m_ub, nx, m_eq)
TALL_MEMBER = (56, 24, 0)
TALL_EQ_MEMBER = (56, 24, 3)
SPREADS = (0.0, 0.5, 1.0, 1.5)        # member i draws its magnitudes over 10^(+-SPREADS[i % 4]): the counts differ inside a batch


def eq_member(seed, m, nx, me, i, own=False):
    """Member i of a family of planted LPs min c^T x, X x <= b, A_eq x = b_eq, x >= 0 over ONE pair (X, A_eq) ~ N(0, 1) (own:
    each member draws its own pair), a strictly complementary vertex as planted_eq plants it, with the primal and dual
    magnitudes of member i spread over 10^(+-SPREADS[i % 4]).  Row 0 of X is all ones and never active: b[0] < 0 makes a member
    infeasible without touching the matrix.  A member depends on (seed, shape, i) alone, whatever the count of its batch.
    -> X, b, A_eq, b_eq, c"""
    r = np.random.default_rng([seed, m, nx, me, i + 1] if own else [seed, m, nx, me])
    X = r.standard_normal((m, nx)); X[0, :] = 1.0
    Ae = r.standard_normal((me, nx))
    r = np.random.default_rng([seed, m, nx, me, i + 1, 77])
    mag = lambda size: 10.0 ** (SPREADS[i % 4] * r.uniform(-1.0, 1.0, size))
    k = min(nx, max(nx // 2, me))
    na = max(k - me, 0)
    xs = np.zeros(nx); xs[r.permutation(nx)[:k]] = mag(k)
    act = 1 + r.permutation(m - 1)[:na]
    sl = mag(m); sl[act] = 0.0
    lam = np.zeros(m); lam[act] = mag(na)
    mu = mag(nx); mu[xs > 0] = 0.0
    c = -X.T @ lam + Ae.T @ r.standard_normal(me) + mu
    return X, X @ xs + sl, Ae, Ae @ xs, c


def dense_own_member(k):
    """Member k of the dense batches whose members own their matrices: 24 x 56, its own A, magnitudes spread by SPREADS[k % 4].
    -> A, b, c"""
    from lp_amd import synth
    A, bs, cs, _ = synth.spread_scenarios(MEMBER_SEED + k, 24, 56, [SPREADS[k % 4]])
    return A, bs[0], cs[0]


def gamma(k):
    """The constant of the standard summation bound: k eps / (1 - k eps)."""
    return k * EPS / (1.0 - k * EPS)


def case_arrays(case):
    """-> dict(A, b, c in slack form; parts (X, b_ub, A_eq, b_eq, c_x) or None; n_slack)."""
    if case[0] == "planted":
        from lp_amd import synth
        A, b, c, xs = synth.planted_lp(PLANTED_SEED, case[1], case[2])
        return dict(A=A, b=b, c=c, parts=None, n_slack=0, xstar=xs)
    X, b, Ae, be, c, xs = planted_eq(*case[1:])
    A, bb, cc = slack_form(X, b, Ae, be, c)
    return dict(A=A, b=bb, c=cc, parts=(X, b, Ae, be, c), n_slack=X.shape[0], xstar=xs)


def permuted_arrays(case):
    """The same LP with its (structural) columns permuted: -> (A', b, c', perm over all n columns: x' = x[perm])."""
    d = case_arrays(case)
    n = d["A"].shape[1]
    if case[0] == "planted":
        perm = np.random.default_rng(7000 + PLANTED_SEED).permutation(n)
        return np.ascontiguousarray(d["A"][:, perm]), d["b"], d["c"][perm], perm
    X, b, Ae, be, c = d["parts"]
    Xp, Aep, cp, p = permuted(X, Ae, c, case[1])
    A, bb, cc = slack_form(Xp, b, Aep, be, cp)
    return A, bb, cc, np.concatenate([p, np.arange(X.shape[1], n)])


def oracle_duals(A, b, c, **opt_kw):
    """The oracle's solve, and its final iterate rebuilt by looping oracle.iteration from the blind start (x = z = 1, y = 0,
    tau = kappa = 1; `ip` on the first pass only) for exactly the iterations the solve reports.
    -> dict(status, iterations, x_slack, fun, log, x_loop = x / tau of the loop, y = y / tau, z = z / tau, tau, kappa)."""
    from oracle import capi as oracle
    opts = oracle.default_opts(**opt_kw)
    ref = oracle.solve(A, b, c, opts=opts)
    m, n = A.shape
    x, y, z, tau, kappa = np.ones(n), np.zeros(m), np.ones(n), 1.0, 1.0
    for k in range(ref["iterations"]):
        r = oracle.iteration(A, b, c, x, y, z, tau, kappa, ip=bool(opts.ip) and k == 0, alpha0=opts.alpha0,
                             solver_type=opts.solver_type)
        x, y, z, tau, kappa = r["x"], r["y"], r["z"], r["tau"], r["kappa"]
    out = dict(ref, x_loop=x / tau, y=y / tau, z=z / tau, tau=tau, kappa=kappa)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_pair(case):
    """oracle_duals of the case as generated and with permuted columns (z mapped back): computed once, shared, read-only."""
    d = case_arrays(case)
    ref = oracle_duals(d["A"], d["b"], d["c"])
    Ap, bp, cp, perm = permuted_arrays(case)
    alt = dict(oracle_duals(Ap, bp, cp))
    for k in ("z", "x_loop", "x_slack"):
        back = np.empty_like(alt[k])
        back[perm] = alt[k]
        back.setflags(write=False)
        alt[k] = back
    return ref, alt


def planted_multipliers(case):
    """y*, z* of a planted (strictly complementary, nondegenerate) LP from the caller's own arrays: the basis is where x* > 0,
    A_B^T y* = c_B, z* = c - A^T y*."""
    d = case_arrays(case)
    A, c, xs = d["A"], d["c"], d["xstar"]
    B = np.flatnonzero(xs > 0)
    assert B.shape[0] == A.shape[0]
    y = np.linalg.solve(A[:, B].T, c[B])
    return y, c - A.T @ y


def check_identities(A, b, c, c0, x, fun, d, row, what, norm_c=None, col_exp=None):
    """The three identities between the duals d = dict(y, z, dual_fun, tau, kappa) of a solve, its x / tau, its fun and the last
    row (alpha, rho_p, rho_d, rho_A, rho_g, rho_mu, obj) of its iteration log, each side recomputed here from A, b, c.
    Allowance: the standard summation bound, 2 gamma_k sum|terms| with k = number of terms + 2, once per side.
      1. |c - A^T y - z|_2 = rho_d max(1, |c - 1|_2) / tau       (r_D = c tau - A^T y - z; rho_d0 = |c - 1|_2 at the blind start)
      2. |fun - dual_fun|  = rho_A (1 + |dual_fun - c0|)          (rho_A = |c.x - b.y| / (tau + |b.y|))
      3. tau^2 x^T z + tau kappa = rho_mu (n + 1)                 (mu_0 = 1 at the blind start)
    A scaled solve (lpipm_set_scaling): the log refers to the scaled problem, whose dual residual is the caller's taken column by
    column by 2^kc[j] (c_j, (A^T y)_j and z_j all carry 2^-kc[j]).  Identity 1 then reads |ldexp(c - A^T y - z, kc)|_2 =
    rho_d norm_c / tau with A, b, c, y, z the caller's, col_exp = kc and norm_c = max(1, |c_scaled - 1|_2).  rho_A or rho_mu
    None in `row`: that identity is not looked at."""
    m, n = A.shape
    y, z, tau, kappa = d["y"], d["z"], d["tau"], d["kappa"]
    _, _, rho_d, rho_A, _, rho_mu, _ = row
    assert tau > 0 and (z > 0).all(), what
    # 1
    kc = np.zeros(n, dtype=np.int32) if col_exp is None else col_exp
    lhs = np.linalg.norm(np.ldexp(c - A.T @ y - z, kc))
    mag = np.linalg.norm(np.ldexp(np.abs(c) + np.abs(A).T @ np.abs(y) + np.abs(z), kc))
    nc = max(1.0, np.linalg.norm(c - 1.0)) if norm_c is None else norm_c
    rhs = rho_d * nc / tau
    tol = 4.0 * gamma(m + 2 + n + 2) * mag
    print(f"\n[measure] {what}: identity 1 |lhs - rhs| {abs(lhs - rhs):.3g} (lhs {lhs:.3g}, allowance {tol:.3g})")
    assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)
    if rho_A is not None:
        lhs = abs(fun - d["dual_fun"])
        mag = np.abs(c) @ np.abs(x) + np.abs(b) @ np.abs(y) + 2.0 * abs(c0)
        rhs = rho_A * (1.0 + abs(d["dual_fun"] - c0))
        tol = 4.0 * gamma(n + m + 2 + 2) * mag
        print(f"[measure] {what}: identity 2 |lhs - rhs| {abs(lhs - rhs):.3g} (lhs {lhs:.3g}, allowance {tol:.3g})")
        assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)
    if rho_mu is not None:
        lhs = tau * tau * (x @ z) + tau * kappa
        rhs = rho_mu * (n + 1)
        tol = 4.0 * gamma(n + 1 + 2) * lhs            # (every term is positive: sum|terms| is the value)
        print(f"[measure] {what}: identity 3 |lhs - rhs| {abs(lhs - rhs):.3g} (lhs {lhs:.3g}, allowance {tol:.3g})")
        assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)


# ---- the oracle's duals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_loop_rebuilds_the_oracles_solve(built, case):
    """The construction proves itself: x / tau of the looped iterate is the solve's x_slack, bit for bit."""
    ref, alt = oracle_pair(case)
    assert ref["status"] == 0 and alt["status"] == 0
    diff = np.abs(ref["x_loop"] - ref["x_slack"]).max()
    print(f"\n[measure] {case}: {ref['iterations']} iterations, max|x_loop - x_slack| {diff:.3g}")
    assert ref["x_loop"].tobytes() == ref["x_slack"].tobytes()
    assert alt["x_loop"].tobytes() == alt["x_slack"].tobytes()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_identities_hold_for_the_oracle(built, case):
    d = case_arrays(case)
    ref, _ = oracle_pair(case)
    dual_fun = float(d["b"] @ ref["y"])
    check_identities(d["A"], d["b"], d["c"], 0.0, ref["x_slack"], ref["fun"], dict(ref, dual_fun=dual_fun), ref["log"][-1],
                     f"oracle {case}")


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_the_oracles_duals_are_stable_under_a_column_permutation(built, case):
    """A condition on the GPU parity inputs: equal counts, and y / tau, z / tau within X_TOL of each other."""
    ref, alt = oracle_pair(case)
    assert ref["iterations"] == alt["iterations"]
    assert ref["status"] == 0 and alt["status"] == 0
    spread = max(np.abs(ref["y"] - alt["y"]).max(), np.abs(ref["z"] - alt["z"]).max())
    print(f"\n[measure] {case}: oracle spread of the duals under a column permutation {spread:.3g}")
    assert spread <= X_TOL, spread


@pytest.mark.parametrize("case", CASES[:3], ids=IDS[:3])
def test_the_oracle_ends_near_the_planted_multipliers(built, case):
    ys, zs = planted_multipliers(case)
    ref, _ = oracle_pair(case)
    dist = max(np.abs(ref["y"] - ys).max(), np.abs(ref["z"] - zs).max())
    print(f"\n[measure] {case}: the oracle's distance from the planted multipliers {dist:.3g}")
    assert dist <= X_TOL, dist


# ---- Problem.denormalize_duals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m_ub,m_eq", [(5, 3, 2), (4, 0, 3), (6, 4, 0), (1, 1, 1)])
def test_denormalize_duals(built, n, m_ub, m_eq):
    """The shapes of test_problem_builder_matches_oracle_and_reference_shape: rows split as the builder stacks them (`ub` first),
    z cut to the structural columns -- the mirror of denormalize_x_into."""
    import lp_amd
    rng = np.random.default_rng(5)
    p = lp_amd.Problem.target(rng.standard_normal(n))
    if m_ub:
        p = p.ub(rng.standard_normal((m_ub, n)), rng.standard_normal(m_ub))
    if m_eq:
        p = p.eq(rng.standard_normal((m_eq, n)), rng.standard_normal(m_eq))
    prob = p.build()
    y, z = rng.standard_normal(m_ub + m_eq), rng.standard_normal(n + m_ub)
    y_ub, y_eq, rc = prob.denormalize_duals(y, z)
    assert y_ub.shape == (m_ub,) and y_eq.shape == (m_eq,) and rc.shape == (n,)
    assert (y_ub == y[:m_ub]).all() and (y_eq == y[m_ub:]).all() and (rc == z[:n]).all()
    assert rc.shape == prob.denormalize_x_into(z).shape
    y_ub[:] = 0.0; rc[:] = 0.0                                     # copies, as denormalize_x_into returns
    assert (y[:m_ub] != 0.0).all() and (z[:n] != 0.0).all()
    # A^T y + z = c of the slack form restricted to the structural columns: A_ub^T y_ub + A_eq^T y_eq + reduced_costs = c
    A = prob.A()
    assert A.shape == (m_ub + m_eq, n + m_ub)
    assert np.allclose((A.T @ y + z)[:n], (A[:m_ub, :n].T @ y[:m_ub] if m_ub else 0.0) + (A[m_ub:, :n].T @ y[m_ub:] if m_eq else 0.0) + z[:n])


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_struct_and_null_context(built):
    from lp_amd import _capi
    lib = _capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lpipm.h")).read()
    ffi = open(os.path.join(root, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ("lpipm_get_duals", "lpipm_get_duals_device"):
        assert name in _capi.SYMBOLS
        assert f"int {name}(" in header
        assert f"pub fn {name}(" in ffi
        assert getattr(lib, name).restype is C.c_int
    assert "lpipm_dual_info" in header and "pub struct lpipm_dual_info" in ffi
    assert _capi.DualInfo is DualInfo and C.sizeof(DualInfo) == 32
    assert len(lib.lpipm_get_duals.argtypes) == 5 and len(lib.lpipm_get_duals_device.argtypes) == 6
    # a null context is a bad argument, and no device is touched to say so
    y = np.ones(3)
    yp = y.ctypes.data_as(C.POINTER(C.c_double))
    info = DualInfo()
    assert lib.lpipm_get_duals(None, 0, yp, yp, C.byref(info)) == _capi.ERR_BAD_ARGUMENT
    assert lib.lpipm_get_duals_device(None, None, 0, None, 0, None) == _capi.ERR_BAD_ARGUMENT
    assert (y == 1.0).all()


# ---- the members of the GPU bit-identity batches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,own", [(SLACK_MEMBER, False), (SLACK_MEMBER, True), (TALL_MEMBER, False), (TALL_MEMBER, True),
                                       (TALL_EQ_MEMBER, False)], ids=["slack", "slack-own", "tall", "tall-own", "tall-eq"])
def test_the_oracle_solves_the_batch_members(built, shape, own):
    """A condition on the inputs: every member of the largest batch is Ok for the oracle, and the counts differ inside a batch."""
    from oracle import capi as oracle
    counts = []
    for i in range(18):
        X, b, Ae, be, c = eq_member(MEMBER_SEED, *shape, i, own)
        ref = oracle.solve(*slack_form(X, b, Ae, be, c), want_log=False)
        assert ref["status"] == 0, (i, ref["status"])
        counts.append(ref["iterations"])
    print(f"\n[measure] {shape} own={own}: the oracle's iteration counts {counts}")
    assert len(set(counts)) > 1


def test_the_oracle_solves_the_dense_batch_members(built):
    from lp_amd import synth
    from oracle import capi as oracle
    A, bs, cs, _ = synth.spread_scenarios(MEMBER_SEED, 24, 56, [SPREADS[i % 4] for i in range(18)])
    counts = []
    for b, c in zip(bs, cs):
        ref = oracle.solve(A, b, c, want_log=False)
        assert ref["status"] == 0
        counts.append(ref["iterations"])
    print(f"\n[measure] spread_scenarios 24x56: the oracle's iteration counts {counts}")
    assert len(set(counts)) > 1
    counts = []
    for k in range(18):
        ref = oracle.solve(*dense_own_member(k), want_log=False)
        assert ref["status"] == 0
        counts.append(ref["iterations"])
    print(f"[measure] dense_own_member: the oracle's iteration counts {counts}")
    assert len(set(counts[:3])) > 1
