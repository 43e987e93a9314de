"""Infeasibility and unboundedness certificates of the last solve (lpipm_get_certificate), without a device: the
inputs, the oracle's certificate -- its looped final iterate, normalised as the header defines --, the conditions the GPU parity
inputs must meet (the intended status, equal counts and rays within X_TOL under a column permutation, strictly positive z^ and
x^), the two identities that tie a ray to the last row of the iteration log, Problem.denormalize_certificate, the new symbols.

The inputs, the oracle construction and the numpy checks of tests/test_gpu_certificates.py live here.

An Unbounded call that proves nothing (status 6 with c.x >= 0).  indicators.rs:72 calls a problem Unbounded whenever the exit
test passes with b.y <= tol, whatever c.x is.  The LPs that are both primal and dual infeasible were searched on the CPU oracle
(find_unproved_unbounded below: min -x1 s.t. x1 - x2 = 0, x3 = -1 and variants of it with a random row, seeds 0 .. 199): 189
of them end with status 5, and the 11 that end with status 6 do so with c.x < 0, a ray that does prove the dual infeasible.  None
makes the oracle report 6 with c.x >= 0, so no such instance is pinned; the NONE branch is tested through Ok and
iteration-limit members."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from lp_amd._capi import CertInfo        # (lpipm_cert_info: without the getter's ABI nothing in this file has a subject)
from test_duals_host import MEMBER_SEED, X_TOL, eq_member, gamma
from test_tall_eq_host import permuted, slack_form

OK, INFEASIBLE, UNBOUNDED, ITERATION_LIMIT = 0, 5, 6, 7
NONE, FARKAS, RAY = 0, 1, 2

# (form, shape): the smallest shapes at which every kernel variant is reached.  dense: the planted LP of shape[0] x shape[1]
# with the extra row 1^T (tests/test_after_a_failed_solve_host.py: 25 x 56 and 131 x 300 -- m no multiple of 128, n no multiple
# of 16, more than one workgroup per member); the others: eq_member(MEMBER_SEED, m_ub, nx, m_eq, member); tallX: shared_X of
# tests/test_gpu_tall_batches.py with its member(X, seed).
SHAPES = [("dense", (24, 56)), ("dense", (130, 300)), ("slack", (24, 32, 8)), ("slack", (300, 40, 5)),
          ("tall", (56, 24, 0)), ("tall", (300, 40, 0)), ("tall_eq", (56, 24, 3)), ("tall_eq", (300, 40, 5)), ("tallX", (300, 40, 0))]
CASES = [(form, shape, which) for form, shape in SHAPES for which in ("infeasible", "unbounded")]
IDS = [f"{form}{'x'.join(map(str, shape))}-{which}" for form, shape, which in CASES]
MEMBERS = (0, 1, 2, 3)                 # of the eq_member families: the stability condition is shown on all four


def infeasible_parts(X, b, Ae, be, c):
    """Row 0 of X is >= 0 (eq_member: all ones): b[0] = -1 leaves no x >= 0 with X x <= b."""
    b = b.copy(); b[0] = -1.0
    return X, b, Ae, be, c


def unbounded_parts(X, b, Ae, be, c):
    """Column 0 of X <= 0, column 0 of A_eq = 0, c[0] = -1: x_0 improves for ever and breaks no row."""
    X, Ae, c = X.copy(), Ae.copy(), c.copy()
    X[:, 0] = -np.abs(X[:, 0]); Ae[:, 0] = 0.0; c[0] = -1.0
    return X, b, Ae, be, c


def dense_lp(m, n, which, k=0):
    """Member k of the dense inputs: planted_lp(MEMBER_SEED + k, m, n) with the extra row 1^T x = sum x* -> A (m + 1) x n, b, c.
    infeasible: 1^T x = -1 (the `bad` vectors of test_after_a_failed_solve_host.dense(..., augmented=True)).  unbounded: a
    direction d > 0 drawn in [0.5, 1.5] is made a ray -- column 0 becomes -(A[:, 1:] d[1:]) / d[0] and c[0] such that c.d = -1,
    so A d = 0 --, and b = A x* keeps x* feasible."""
    from test_after_a_failed_solve_host import dense
    fam = dense(MEMBER_SEED + k, m, n, 1, False, True)
    A = fam.mat(0)[0]
    if which == "infeasible":
        return A, fam.vecs["bad"][0][0], fam.vecs["bad"][1][0]
    b, c = fam.vecs["good"][0][0], fam.vecs["good"][1][0]
    if which == "good":
        return A, b, c
    from lp_amd import synth
    xs = synth.planted_lp(MEMBER_SEED + k, m, n)[3]
    A, c = A.copy(), c.copy()
    d = np.random.default_rng([MEMBER_SEED + k, m, n, 99]).uniform(0.5, 1.5, n)
    A[:, 0] = -(A[:, 1:] @ d[1:]) / d[0]; c[0] = (-1.0 - c[1:] @ d[1:]) / d[0]
    return A, A @ xs, c


# ---- the members of the GPU bit-identity batches: tests/test_duals_host.py's shapes, member `role(k, K)` of a batch of K -------------
DENSE_MEMBER = (24, 56)                # a 25 x 56 LP
BATCH_KINDS = ["dense", "dense-own", "slack", "slack-own", "tall", "tall-own", "tall-eq"]


def role(k, K):
    """An infeasible member at position 1, an unbounded one last, good ones elsewhere."""
    return "infeasible" if k == 1 else "unbounded" if k == K - 1 else "good"


def dense_member(k, which, own=False):
    """Member k of the dense batches, 25 x 56: G = [A; 1^T] with A = planted_lp(MEMBER_SEED (own: + k), 24, 56)'s matrix and
    column 0 of G zeroed, a planted strictly complementary vertex on 25 of the columns 1 .. 55 with magnitudes spread over
    10^(+-SPREADS[k % 4]) as spread_scenarios spreads them.  Row 24 is (0, 1, ..., 1): b[24] = -1 makes a member infeasible
    through b alone; column 0 meets no row: c[0] = -1 makes a member unbounded through c alone (a good member has c[0] > 0).
    -> G, b, c"""
    from lp_amd import synth
    from test_duals_host import SPREADS
    m, n = DENSE_MEMBER
    G = np.vstack([synth.planted_lp(MEMBER_SEED + (k if own else 0), m, n)[0], np.ones(n)])
    G[:, 0] = 0.0
    r = np.random.default_rng([MEMBER_SEED, m, n, k, 31])
    sp = SPREADS[k % 4]
    basis = 1 + r.permutation(n - 1)[:m + 1]
    x, z = np.zeros(n), 10.0 ** (sp * r.uniform(-1.0, 1.0, n))
    x[basis] = 10.0 ** (sp * r.uniform(-1.0, 1.0, m + 1)); z[basis] = 0.0
    b, c = G @ x, G.T @ r.standard_normal(m + 1) + z
    if which == "infeasible":
        b[m] = -1.0
    elif which == "unbounded":
        c[0] = -1.0
    return G, b, c


def batch_member(kind, k, which):
    """Member k of a bit-identity batch in the role `which` -> dense kinds: (A, b, c); the others: (X, b, A_eq, b_eq, c)."""
    from test_duals_host import SLACK_MEMBER, TALL_EQ_MEMBER, TALL_MEMBER
    own = kind.endswith("-own")
    if kind.startswith("dense"):
        return dense_member(k, which, own)
    shape = {"slack": SLACK_MEMBER, "tall": TALL_MEMBER, "tall-eq": TALL_EQ_MEMBER}[kind.removesuffix("-own")]
    X, b, Ae, be, c = eq_member(MEMBER_SEED, *shape, k, own)
    if not own:        # one pair (X, A_eq) for the whole batch: the unbounded member's matrix is everybody's -- column 0 <= 0 in X
        X, Ae, c = X.copy(), Ae.copy(), c.copy()          # (0 in row 0, which stays >= 0) and 0 in A_eq; a member that is not
        X[:, 0] = -np.abs(X[:, 0]); X[0, 0] = 0.0; Ae[:, 0] = 0.0      # to be unbounded pays for x_0: c[0] = 0.5
        c[0] = 0.5
        b, be = b_of_shared(shape, k, X, Ae)
    if which == "infeasible":
        return infeasible_parts(X, b, Ae, be, c)
    if which == "unbounded":
        return unbounded_parts(X, b, Ae, be, c)
    return X, b, Ae, be, c


def b_of_shared(shape, k, X, Ae):
    """eq_member's right-hand sides on the shared pair whose column 0 was changed: X x* + slack and A_eq x* with eq_member's
    own x* (recovered from its draws) and slacks (b - X0 x*).  -> b, b_eq"""
    r = np.random.default_rng([MEMBER_SEED, *shape])
    m, nx, me = shape
    X0 = r.standard_normal((m, nx)); X0[0, :] = 1.0
    _, b0, Ae0, be0, _ = eq_member(MEMBER_SEED, *shape, k)
    from test_duals_host import SPREADS
    r = np.random.default_rng([MEMBER_SEED, m, nx, me, k + 1, 77])
    mag = lambda size: 10.0 ** (SPREADS[k % 4] * r.uniform(-1.0, 1.0, size))
    kk = min(nx, max(nx // 2, me))
    xs = np.zeros(nx); xs[r.permutation(nx)[:kk]] = mag(kk)
    assert np.array_equal(Ae0 @ xs, be0)                            # the draws are eq_member's
    return b0 - X0 @ xs + X @ xs, Ae @ xs


def parts_of(form, shape, which, k=0):
    """-> X, b, A_eq, b_eq, c of member k of a form that is given in parts."""
    if form == "tallX":
        import test_gpu_tall_batches as gen
        X = gen.shared_X(100 + shape[0], shape[0], shape[1])
        b, c = gen.member(X, 40 + k)
        b, c = b.copy(), c.copy()
        if which == "infeasible":
            b[0] = -1.0
        elif which == "unbounded":
            c[0] = -1.0
        return X, b, np.zeros((0, shape[1])), np.zeros(0), c
    p = eq_member(MEMBER_SEED, *shape, k)
    return {"infeasible": infeasible_parts, "unbounded": unbounded_parts, "good": lambda *q: q}[which](*p)


def case_lp(case, k=0):
    """-> dict(A, b, c: the slack form the oracle solves; parts or None)."""
    form, shape, which = case
    if form == "dense":
        A, b, c = dense_lp(*shape, which, k)
        return dict(A=A, b=b, c=c, parts=None)
    parts = parts_of(form, shape, which, k)
    A, b, c = slack_form(*parts)
    return dict(A=A, b=b, c=c, parts=parts)


def permuted_lp(case, k=0):
    """The same LP with its (structural) columns permuted -> A', b, c', perm over all n columns (x' = x[perm])."""
    d = case_lp(case, k)
    n = d["A"].shape[1]
    if d["parts"] is None:
        perm = np.random.default_rng(7100 + n).permutation(n)
        return np.ascontiguousarray(d["A"][:, perm]), d["b"], d["c"][perm], perm
    X, b, Ae, be, c = d["parts"]
    Xp, Aep, cp, p = permuted(X, Ae, c, X.shape[0])
    A, bb, cc = slack_form(Xp, b, Aep, be, cp)
    return A, bb, cc, np.concatenate([p, np.arange(X.shape[1], n)])


def normalise(status, b, c, x, y, z):
    """The header's definition on a homogeneous iterate -> kind, scale, y^ | None, col | None."""
    if status == INFEASIBLE:
        s = float(b @ y)
        return FARKAS, s, y / s, z / s
    if status == UNBOUNDED:
        s = -float(c @ x)
        return (RAY, s, None, x / s) if s > 0 else (NONE, s, None, None)
    return NONE, np.nan, None, None


def oracle_certificate(A, b, c, **opt_kw):
    """The oracle's solve, its final iterate rebuilt by looping oracle.iteration from the blind start for exactly the iterations
    the solve reports (tests/test_duals_host.py::oracle_duals), normalised as the header defines.
    -> dict(status, iterations, log, x, y, z, tau, kappa: the homogeneous iterate; kind, scale, yh, col)."""
    from oracle import capi as oracle
    opts = oracle.default_opts(**opt_kw)
    ref = oracle.solve(A, b, c, opts=opts)
    m, n = A.shape
    x, y, z, tau, kappa = np.ones(n), np.zeros(m), np.ones(n), 1.0, 1.0
    for k in range(ref["iterations"]):
        r = oracle.iteration(A, b, c, x, y, z, tau, kappa, ip=bool(opts.ip) and k == 0, alpha0=opts.alpha0,
                             solver_type=opts.solver_type)
        x, y, z, tau, kappa = r["x"], r["y"], r["z"], r["tau"], r["kappa"]
    kind, scale, yh, col = normalise(ref["status"], b, c, x, y, z)
    out = dict(status=ref["status"], iterations=ref["iterations"], log=ref["log"], x=x, y=y, z=z, tau=tau, kappa=kappa,
               kind=kind, scale=scale, yh=yh, col=col)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_pair(case, k=0):
    """oracle_certificate of the case as generated and with permuted columns (col mapped back): computed once, read-only."""
    d = case_lp(case, k)
    ref = oracle_certificate(d["A"], d["b"], d["c"])
    Ap, bp, cp, perm = permuted_lp(case, k)
    alt = dict(oracle_certificate(Ap, bp, cp))
    if alt["col"] is not None:
        back = np.empty_like(alt["col"])
        back[perm] = alt["col"]
        back.setflags(write=False)
        alt["col"] = back
    return ref, alt


def want_status(case):
    return INFEASIBLE if case[2] == "infeasible" else UNBOUNDED


def check_certificate(A, b, c, cert, what, kr=None, kc=None):
    """The numpy checks of a certificate dict(kind, y, col, scale, residual) against the caller's own A, b, c, each bound the
    standard summation bound 4 gamma_k sum|terms|: the sign condition exactly, the normalisation |b.y^ - 1| or |c.x^ + 1|, and
    `residual` against the recomputation of its definition.  -> the recomputed residual"""
    m, n = A.shape
    g = 4.0 * gamma(m + n + 4)
    if cert["kind"] == FARKAS:
        y, z = cert["y"], cert["col"]
        assert (z >= 0).all(), what
        norm, mag = abs(float(b @ y) - 1.0), float(np.abs(b) @ np.abs(y)) + 1.0
        res = float(np.abs(A.T @ y + z).max())
        bound = g * float((np.abs(A).T @ np.abs(y) + np.abs(z)).max())
    else:
        assert cert["kind"] == RAY, what
        x = cert["col"]
        assert (x >= 0).all(), what
        norm, mag = abs(float(c @ x) + 1.0), float(np.abs(c) @ np.abs(x)) + 1.0
        res = float(np.abs(A @ x).max())
        bound = g * float((np.abs(A) @ np.abs(x)).max())
    print(f"\n[measure] {what}: kind {cert['kind']}, normalisation off by {norm:.3g} (allowance {g * mag:.3g}), residual "
          f"{cert['residual']:.3g}, |residual - numpy's| {abs(cert['residual'] - res):.3g} (allowance {bound:.3g})")
    assert norm <= g * mag, (what, norm, g * mag)
    assert abs(cert["residual"] - res) <= bound, (what, cert["residual"], res, bound)
    return res


def check_ray_identities(A, b, c, cert, row, what, norm_b=None, norm_c=None, row_exp=None, col_exp=None):
    """The identity between a certificate dict(kind, y, col, scale, tau) and the last row (alpha, rho_p, rho_d, ...) of the
    iteration log of its solve, both sides recomputed from A, b, c:
      (a) Farkas: |A^T y^ + z^ - c tau / s|_2 = rho_d max(1, |c - 1|_2) / s      (r_D = c tau - A^T y - z over s)
      (b) ray:    |A x^ - b tau / s|_2       = rho_p max(1, |b - A 1|_2) / s      (r_P = b tau - A x over s)
    Allowance: 4 gamma_k sum|terms|, as check_identities of tests/test_duals_host.py.  A scaled solve: the log is the scaled
    problem's, whose residuals are the caller's taken by 2^kc[j] per column, respectively 2^kr[i] per row; norm_b / norm_c are
    the scaled problem's max(1, |.|)."""
    m, n = A.shape
    tau, s = cert["tau"], cert["scale"]
    _, rho_p, rho_d = row[:3]
    if cert["kind"] == FARKAS:
        kc = np.zeros(n, dtype=np.int32) if col_exp is None else col_exp
        y, z = cert["y"], cert["col"]
        lhs = np.linalg.norm(np.ldexp(A.T @ y + z - c * (tau / s), kc))
        mag = np.linalg.norm(np.ldexp(np.abs(A).T @ np.abs(y) + np.abs(z) + np.abs(c) * (tau / s), kc))
        rhs = rho_d * (max(1.0, np.linalg.norm(c - 1.0)) if norm_c is None else norm_c) / s
    else:
        kr = np.zeros(m, dtype=np.int32) if row_exp is None else row_exp
        x = cert["col"]
        lhs = np.linalg.norm(np.ldexp(A @ x - b * (tau / s), kr))
        mag = np.linalg.norm(np.ldexp(np.abs(A) @ np.abs(x) + np.abs(b) * (tau / s), kr))
        rhs = rho_p * (max(1.0, np.linalg.norm(b - A @ np.ones(n))) if norm_b is None else norm_b) / s
    tol = 4.0 * gamma(m + n + 4) * mag
    print(f"[measure] {what}: identity ({'a' if cert['kind'] == FARKAS else 'b'}) |lhs - rhs| {abs(lhs - rhs):.3g} "
          f"(lhs {lhs:.3g}, allowance {tol:.3g})")
    assert abs(lhs - rhs) <= tol, (what, lhs, rhs, tol)


# ---- the oracle's certificates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_ends_as_intended_and_its_ray_is_stable(built, case):
    """Conditions on the GPU parity inputs: the intended status on the LP as generated and with permuted columns, equal counts,
    rays within X_TOL of each other, strictly positive z^ / x^, and a residual that makes the ray a certificate."""
    members = MEMBERS if case[0] in ("slack", "tall", "tall_eq") else (0,)
    for k in members:
        ref, alt = oracle_pair(case, k)
        assert ref["status"] == alt["status"] == want_status(case), (k, ref["status"], alt["status"])
        assert ref["iterations"] == alt["iterations"], (k, ref["iterations"], alt["iterations"])
        assert ref["kind"] == alt["kind"] == (FARKAS if case[2] == "infeasible" else RAY) and ref["scale"] > 0
        spread = np.abs(ref["col"] - alt["col"]).max()
        if ref["kind"] == FARKAS:
            spread = max(spread, np.abs(ref["yh"] - alt["yh"]).max())
        d = case_lp(case, k)
        res = np.abs(d["A"].T @ ref["yh"] + ref["col"]).max() if ref["kind"] == FARKAS else np.abs(d["A"] @ ref["col"]).max()
        print(f"\n[measure] {case} member {k}: status {ref['status']} after {ref['iterations']} iterations, spread of the ray under "
              f"a column permutation {spread:.3g}, residual {res:.3g}, largest entry {np.abs(ref['col']).max():.3g}")
        assert spread <= X_TOL, (k, spread)
        assert (ref["col"] > 0).all() and (alt["col"] > 0).all()
        assert res <= X_TOL, (k, res)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ray_identities_hold_for_the_oracle(built, case):
    d = case_lp(case)
    ref, _ = oracle_pair(case)
    cert = dict(kind=ref["kind"], y=ref["yh"], col=ref["col"], scale=ref["scale"], tau=ref["tau"])
    check_ray_identities(d["A"], d["b"], d["c"], cert, ref["log"][-1], f"oracle {case}")
    res = np.abs(d["A"].T @ ref["yh"] + ref["col"]).max() if ref["kind"] == FARKAS else np.abs(d["A"] @ ref["col"]).max()
    check_certificate(d["A"], d["b"], d["c"], dict(cert, residual=float(res)), f"oracle {case}")


@functools.lru_cache(maxsize=None)
def batch_oracle(kind, K):
    """(status, iterations) of the oracle on every member of the bit-identity batch of K."""
    from oracle import capi as oracle
    out = []
    for k in range(K):
        mem = batch_member(kind, k, role(k, K))
        ref = oracle.solve(*(mem if len(mem) == 3 else slack_form(*mem)), want_log=False)
        out.append((ref["status"], ref["iterations"]))
    return out


def limit_for(results):
    """The iteration limit of a bit-identity batch from its members' (status, iterations) under the default options: the count
    of the unbounded (last) member, so that it and the infeasible member still end as they do, at least one good member
    finishes and -- at 16 and 18 members -- at least one good member is stopped at the limit."""
    return results[-1][1]


@pytest.mark.parametrize("K", [3, 16, 18])
@pytest.mark.parametrize("kind", BATCH_KINDS)
def test_the_oracle_ends_the_batch_members_as_intended(built, kind, K):
    """A condition on the inputs of the bit-identity batches: member 1 infeasible, the last unbounded, every other Ok; the
    infeasible member ends no later than the unbounded one; at 16 and 18 members the limit leaves good members on both sides."""
    res = batch_oracle(kind, K)
    print(f"\n[measure] {kind} x {K}: the oracle's (status, iterations) {res}")
    assert [st for st, _ in res] == [{"infeasible": INFEASIBLE, "unbounded": UNBOUNDED, "good": OK}[role(k, K)] for k in range(K)]
    L = limit_for(res)
    assert res[1][1] <= L
    good = [it for k, (_, it) in enumerate(res) if role(k, K) == "good"]
    assert K == 3 or (min(good) <= L < max(good)), (L, good)


def find_unproved_unbounded(seeds=range(200)):
    """The search the module docstring reports: LPs that are both primal and dual infeasible -- min -x1 s.t. x1 - x2 = 0,
    x3 = -1, and the same with a random third row and two more columns --, looking for status 6 with c.x >= 0.
    -> list of (seed, status, c.x) of the instances that end Unbounded with c.x >= 0."""
    found = []
    for seed in seeds:
        r = np.random.default_rng(seed)
        if seed == 0:
            A, b, c = np.array([[1.0, -1.0, 0.0], [0.0, 0.0, 1.0]]), np.array([0.0, -1.0]), np.array([-1.0, 0.0, 0.0])
        else:
            A = np.zeros((3, 5)); A[0, :2] = [1.0, -1.0]; A[1, 2] = 1.0; A[2, 2:] = np.abs(r.standard_normal(3))
            b = np.array([0.0, -1.0, -r.uniform(0.5, 2.0)])
            c = np.concatenate([[-1.0, 0.0], r.uniform(0.0, 1.0, 3)])
        ref = oracle_certificate(A, b, c)
        if ref["status"] == UNBOUNDED and float(c @ ref["x"]) >= 0.0:
            found.append((seed, ref["status"], float(c @ ref["x"])))
    return found


def test_no_small_instance_is_unbounded_without_a_ray(built):
    """(What the module docstring says: if this ever finds one, pin it and test the NONE branch of an Unbounded member with it.)"""
    assert find_unproved_unbounded(range(40)) == []


# ---- Problem.denormalize_certificate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m_ub,m_eq", [(5, 3, 2), (4, 0, 3), (6, 4, 0), (1, 1, 1)])
def test_denormalize_certificate(built, n, m_ub, m_eq):
    import lp_amd
    rng = np.random.default_rng(5)
    p = lp_amd.Problem.target(rng.standard_normal(n))
    if m_ub:
        p = p.ub(rng.standard_normal((m_ub, n)), rng.standard_normal(m_ub))
    if m_eq:
        p = p.eq(rng.standard_normal((m_eq, n)), rng.standard_normal(m_eq))
    prob = p.build()
    y, col = rng.standard_normal(m_ub + m_eq), rng.standard_normal(n + m_ub)
    y_ub, y_eq, z = prob.denormalize_certificate(y, col, FARKAS)
    assert y_ub.shape == (m_ub,) and y_eq.shape == (m_eq,) and z.shape == (n,)
    assert (y_ub == y[:m_ub]).all() and (y_eq == y[m_ub:]).all() and (z == col[:n]).all()
    assert prob.denormalize_duals(y, col)[0].tobytes() == y_ub.tobytes()          # the mirror of denormalize_duals
    y_ub[:] = 0.0; z[:] = 0.0                                                      # copies
    assert (y[:m_ub] != 0.0).all() and (col[:n] != 0.0).all()
    a, b_, x = prob.denormalize_certificate(None, col, RAY)
    assert a is None and b_ is None and x.shape == (n,) and (x == col[:n]).all()
    x[:] = 0.0
    assert (col[:n] != 0.0).all()
    assert prob.denormalize_certificate(y, col, NONE) == (None, None, None)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_struct_and_null_context(built):
    from lp_amd import _capi
    lib = _capi.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lpipm.h")).read()
    ffi = open(os.path.join(root, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ("lpipm_get_certificate", "lpipm_get_certificate_device"):
        assert name in _capi.SYMBOLS
        assert f"int {name}(" in header
        assert f"pub fn {name}(" in ffi
        assert getattr(lib, name).restype is C.c_int
    assert "lpipm_cert_info" in header and "pub struct lpipm_cert_info" in ffi
    assert _capi.CertInfo is CertInfo and C.sizeof(CertInfo) == 40
    assert (_capi.CERT_NONE, _capi.CERT_FARKAS, _capi.CERT_RAY) == (NONE, FARKAS, RAY)
    assert len(lib.lpipm_get_certificate.argtypes) == 5 and len(lib.lpipm_get_certificate_device.argtypes) == 6
    # a null context is a bad argument, and no device is touched to say so; nothing is written
    y = np.ones(3)
    yp = y.ctypes.data_as(C.POINTER(C.c_double))
    info = CertInfo(-7.0, -7.0, -7.0, -7.0, -7, -7)
    assert lib.lpipm_get_certificate(None, 0, yp, yp, C.byref(info)) == _capi.ERR_BAD_ARGUMENT
    assert lib.lpipm_get_certificate_device(None, None, 0, None, 0, C.byref(info)) == _capi.ERR_BAD_ARGUMENT
    assert (y == 1.0).all() and info.kind == -7 and info.status == -7 and info.scale == -7.0
