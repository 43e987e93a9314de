"""Dual values and reduced costs of the last solve (lpipm_get_duals, lpipm_get_duals_device) on the device:
parity with the oracle's duals, the identities that tie them to the logged indicators, bit-identity of every member across
every resident form, count and entry, the tall forms against the slack form, scaling, validity and refusals, a getter that
leaves nothing behind, the Python drivers.  Inputs, oracle construction and identity checks: tests/test_duals_host.py."""
import ctypes as C

import numpy as np
import pytest

from test_duals_host import (ALL_CASES, ALL_IDS, CASES, IDS, MEMBER_SEED, SLACK_MEMBER, SPREADS, TALL_EQ_MEMBER, TALL_MEMBER, X_TOL,
                             case_arrays, check_identities, dense_own_member, eq_member, oracle_pair, planted_multipliers)
from test_tall_eq_host import planted_eq, slack_form

pytestmark = pytest.mark.gpu

OK, INFEASIBLE, ITERATION_LIMIT = 0, 5, 7
NO_PROBLEM, BAD_ARGUMENT = 101, 103
KEYS = ("y", "z", "dual_fun", "tau", "kappa")


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _problem(X, b, Ae, be, c):
    import lp_amd
    p = lp_amd.Problem.target(c).ub(X, b)
    return (p.eq(Ae, be) if Ae.shape[0] else p).build()


def _bits(d):
    """The duals of one member as bytes (None stays None)."""
    if d is None:
        return None
    return tuple(np.ascontiguousarray(d[k], dtype=np.float64).tobytes() for k in KEYS)


def _duals_or_none(cx, member=0):
    import lp_amd
    try:
        return cx.duals(member)
    except lp_amd.LinearProgramError:
        return None


def _raw_get(cx, member, m, n):
    """lpipm_get_duals itself: -> (rc, y, z, info) with sentinel-filled outputs."""
    from lp_amd import _capi
    y, z = np.full(m, -7.0), np.full(n, -7.0)
    info = _capi.DualInfo(-7.0, -7.0, -7.0, -7, 0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = _capi.lib().lpipm_get_duals(cx._h, member, dp(y), dp(z), C.byref(info))
    return rc, y, z, info


def _upload_case(cx, case, how=None):
    """The upload the parity test names for the case: planted -> lpipm_upload; eq -> lpipm_upload_ub_eq, or how = "slack":
    lpipm_upload_slack on the slack form with its hint; "tall": lpipm_upload_ub_tall / lpipm_upload_ub_eq_tall."""
    d = case_arrays(case)
    if case[0] == "planted":
        return cx.upload_arrays(d["A"], d["b"], d["c"])
    if how == "slack":
        return cx.upload_arrays(d["A"], d["b"], d["c"], 0.0, d["n_slack"])
    prob = _problem(*d["parts"])
    if how == "tall":
        return cx.upload_tall_eq(prob) if d["parts"][2].shape[0] else cx.upload(prob, tall=True)
    return cx.upload(prob)


# ---- 1. oracle parity -------------------------------------------------------------------------------------------------------------
def _check_envelope(case, got, d, what):
    ref, alt = oracle_pair(case)
    rc, x, fun, it, _ = got
    assert ref["status"] == alt["status"] == OK and rc == OK, (what, rc)
    assert it in (ref["iterations"], alt["iterations"]), (what, it, ref["iterations"], alt["iterations"])
    worst = 0.0
    for k in ("y", "z"):
        lo, hi = np.minimum(ref[k], alt[k]), np.maximum(ref[k], alt[k])
        worst = max(worst, np.maximum(np.maximum(lo - d[k], d[k] - hi), 0.0).max())
    print(f"\n[measure] {what}: {it} iterations, duals outside the oracle's envelope by {worst:.3g}")
    assert worst <= X_TOL, (what, worst)
    assert abs(d["dual_fun"] - float(case_arrays(case)["b"] @ ref["y"])) <= 1e-6 * max(1.0, abs(ref["fun"]))


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_duals_match_the_oracle(ctx, case):
    how = "slack" if case[0] == "eq" and case[4] == 0 else None
    _upload_case(ctx, case, how)
    got = ctx.solve_raw(_opts())
    d = ctx.duals()
    a = case_arrays(case)
    assert d["y"].shape == a["b"].shape and d["z"].shape == a["c"].shape
    _check_envelope(case, got, d, f"{case} {how or ''}")
    if case[0] == "planted":
        ys, zs = planted_multipliers(case)
        ref, _ = oracle_pair(case)
        own = max(np.abs(ref["y"] - ys).max(), np.abs(ref["z"] - zs).max())
        dist = max(np.abs(d["y"] - ys).max(), np.abs(d["z"] - zs).max())
        print(f"[measure] {case}: distance from the planted multipliers {dist:.3g} (the oracle's {own:.3g})")
        assert dist <= own + X_TOL


# ---- 2. identities of the logged indicators ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_identities_of_the_logged_indicators(ctx, case):
    a = case_arrays(case)
    c0 = 0.75 if case[0] == "planted" else 0.0
    if case[0] == "planted":
        ctx.upload_arrays(a["A"], a["b"], a["c"], c0)
    else:
        _upload_case(ctx, case)
    rc, x, fun, it, rows = ctx.solve_raw(_opts(), want_log=True)
    assert rc == OK and len(rows) == it
    d = ctx.duals()
    assert d["tau"] > 0 and (d["z"] > 0).all()
    check_identities(a["A"], a["b"], a["c"], c0, x, fun, d, rows[-1], f"gpu {case}")


# ---- 3. bit-identity across paths ---------------------------------------------------------------------------------------------------
def _dense_shared():
    from lp_amd import synth
    return synth.spread_scenarios(MEMBER_SEED, 24, 56, [SPREADS[i % 4] for i in range(18)])[:3]


def _parts(shape, own, k):
    return eq_member(MEMBER_SEED, *shape, k, own)


# form -> (upload of the members [0, K) as one batch, upload of member k alone)
def _form(name):
    if name == "lockstep":
        mem = dense_own_member
        return (lambda cx, K: cx.upload_lockstep(*map(list, zip(*[mem(k) for k in range(K)]))),
                lambda cx, k: cx.upload_arrays(*mem(k)))
    if name == "shared":
        A, bs, cs = _dense_shared()
        return (lambda cx, K: cx.upload_lockstep_shared(A, bs[:K], cs[:K]), lambda cx, k: cx.upload_arrays(A, bs[k], cs[k]))
    if name in ("lockstep_slack", "shared_slack"):
        own = name == "lockstep_slack"
        mem = lambda k: slack_form(*_parts(SLACK_MEMBER, own, k))
        ns = SLACK_MEMBER[0]
        single = lambda cx, k: cx.upload_arrays(*mem(k), 0.0, ns)
        if own:
            return (lambda cx, K: cx.upload_lockstep(*map(list, zip(*[mem(k) for k in range(K)])), n_slack=ns), single)
        return (lambda cx, K: cx.upload_lockstep_shared(mem(0)[0], [mem(k)[1] for k in range(K)], [mem(k)[2] for k in range(K)],
                                                        n_slack=ns), single)
    shape, tall = {"shared_ub_eq": (SLACK_MEMBER, False), "shared_ub_tall": (TALL_MEMBER, True),
                   "shared_ub_eq_tall": (TALL_EQ_MEMBER, True), "lockstep_ub_tall": (TALL_MEMBER, True)}[name]
    own = name == "lockstep_ub_tall"
    mem = lambda k: _parts(shape, own, k)
    bvec = lambda k: np.concatenate([mem(k)[1], mem(k)[3]])

    def single(cx, k):
        prob = _problem(*mem(k))
        if not tall:
            return cx.upload(prob)
        return cx.upload_tall_eq(prob) if shape[2] else cx.upload(prob, tall=True)

    def batch(cx, K):
        X, _, Ae, _, _ = mem(0)
        bs, cs = [bvec(k) for k in range(K)], [mem(k)[4] for k in range(K)]
        if name == "shared_ub_eq":
            return cx.upload_lockstep_shared_ub_eq(X, Ae, bs, cs)
        if name == "shared_ub_tall":
            return cx.upload_lockstep_shared_ub_tall(X, bs, cs)
        if name == "shared_ub_eq_tall":
            return cx.upload_lockstep_shared_ub_eq_tall(X, Ae, bs, cs)
        return cx.upload_lockstep_ub_tall([mem(k)[0] for k in range(K)], bs, cs)
    return batch, single


FORMS = ["lockstep", "lockstep_slack", "shared", "shared_slack", "shared_ub_eq", "shared_ub_tall", "shared_ub_eq_tall",
         "lockstep_ub_tall"]
_singles = {}


def _single_result(ctx, name, k, **okw):
    """Member k of the form alone: upload + lpipm_solve + lpipm_get_duals.  Computed once per (form, member, options)."""
    key = (name, k, tuple(sorted(okw.items())))
    if key not in _singles:
        _form(name)[1](ctx, k)
        rc, x, fun, it, _ = ctx.solve_raw(_opts(**okw))
        _singles[key] = (rc, it, _bits(_duals_or_none(ctx)))
    return _singles[key]


@pytest.mark.parametrize("K", [3, 16, 18])
@pytest.mark.parametrize("name", FORMS)
def test_every_member_has_the_bits_of_its_single_solve(ctx, name, K):
    import torch
    singles = [_single_result(ctx, name, k) for k in range(K)]
    _form(name)[0](ctx, K)
    res = ctx.solve_lockstep(_opts())
    its = [r[3] for r in res]
    assert [r[0] for r in res] == [s[0] for s in singles] and its == [s[1] for s in singles]
    assert all(r[0] == OK for r in res) and len(set(its)) > 1, its          # the members finish at different iterations
    got = ctx.duals_lockstep()
    for k in range(K):
        assert _bits(got[k]) == singles[k][2], (name, K, k)
    # the device entry: the same bits, into rows wider than the vectors; the gaps keep the sentinel
    m, n = ctx.m, ctx.n
    ldy, ldz = m + 3, n + 5
    yd = torch.full((K, ldy), -7.0, dtype=torch.float64, device="cuda")
    zd = torch.full((K, ldz), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    from lp_amd import _capi
    info = (_capi.DualInfo * K)()
    assert _capi.lib().lpipm_get_duals_device(ctx._h, C.c_void_p(yd.data_ptr()), ldy, C.c_void_p(zd.data_ptr()), ldz, info) == OK
    assert ctx.duals_device(None, 0, None, 0) == [(OK, got[k]["dual_fun"]) for k in range(K)]
    yh, zh = yd.cpu().numpy(), zd.cpu().numpy()
    for k in range(K):
        assert info[k].status == OK and info[k].reserved == 0
        assert _bits(dict(got[k], dual_fun=info[k].dual_fun, tau=info[k].tau, kappa=info[k].kappa)) == _bits(got[k])
        assert yh[k, :m].tobytes() == got[k]["y"].tobytes() and zh[k, :n].tobytes() == got[k]["z"].tobytes()
    assert (yh[:, m:] == -7.0).all() and (zh[:, n:] == -7.0).all()


def test_members_without_a_solution_and_at_the_iteration_limit(ctx):
    """A shared_ub_eq batch of 16 (two half-batch views) with one infeasible member (row 0 of X is all ones: b[0] = -1); then
    the same batch stopped at 3 iterations: the members that were not finished are at the limit and have duals."""
    import torch
    from lp_amd import _capi
    K, bad = 16, 9
    mem = [list(_parts(SLACK_MEMBER, False, k)) for k in range(K)]
    mem[bad][1] = mem[bad][1].copy(); mem[bad][1][0] = -1.0
    X, Ae = mem[0][0], mem[0][2]
    bs, cs = [np.concatenate([q[1], q[3]]) for q in mem], [q[4] for q in mem]
    m, n = ctx.upload_lockstep_shared_ub_eq(X, Ae, bs, cs).m, ctx.n
    res = ctx.solve_lockstep(_opts())
    assert [r[0] for r in res] == [INFEASIBLE if k == bad else OK for k in range(K)]
    got = ctx.duals_lockstep()
    assert got[bad] is None
    rc, y, z, info = _raw_get(ctx, bad, m, n)                     # the member's own status, nothing written
    assert rc == INFEASIBLE and (y == -7.0).all() and (z == -7.0).all() and info.status == -7 and info.tau == -7.0
    yd = torch.full((K, m), -7.0, dtype=torch.float64, device="cuda")
    zd = torch.full((K, n), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    infos = (_capi.DualInfo * K)()
    assert _capi.lib().lpipm_get_duals_device(ctx._h, C.c_void_p(yd.data_ptr()), m, C.c_void_p(zd.data_ptr()), n, infos) == OK
    yh, zh = yd.cpu().numpy(), zd.cpu().numpy()
    assert (yh[bad] == -7.0).all() and (zh[bad] == -7.0).all()    # the undelivered member's rows are untouched
    assert infos[bad].status == INFEASIBLE and all(np.isnan(v) for v in (infos[bad].dual_fun, infos[bad].tau, infos[bad].kappa))
    for k in range(K):
        if k == bad:
            continue
        assert _bits(got[k]) == _single_result(ctx, "shared_ub_eq", k)[2], k
    # (the singles above replaced the resident problem: upload again) three iterations: every unfinished member is at the limit
    ctx.upload_lockstep_shared_ub_eq(X, Ae, bs, cs)
    res = ctx.solve_lockstep(_opts(max_iter=3))
    assert ITERATION_LIMIT in [r[0] for r in res]
    got = ctx.duals_lockstep()
    for k in range(K):
        if k == bad:
            continue
        rc1, it1, bits1 = _single_result(ctx, "shared_ub_eq", k, max_iter=3)
        assert (res[k][0], res[k][3]) == (rc1, it1) and rc1 in (OK, ITERATION_LIMIT)
        assert got[k] is not None and _bits(got[k]) == bits1, k


def test_upload_device_gives_the_bits_of_its_host_entry(ctx):
    import torch
    K = 5
    mem = [slack_form(*_parts(SLACK_MEMBER, False, k)) for k in range(K)]
    A, bs, cs = mem[0][0], [q[1] for q in mem], [q[2] for q in mem]
    ns = SLACK_MEMBER[0]
    ctx.upload_lockstep_shared(A, bs, cs, n_slack=ns)
    host_res = ctx.solve_lockstep(_opts())
    host = [_bits(d) for d in ctx.duals_lockstep()]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    ctx.upload_device(t(A), t(np.stack(bs)), t(np.stack(cs)), n_slack=ns)
    dev_res = ctx.solve_lockstep(_opts())
    assert [(r[0], r[3]) for r in dev_res] == [(r[0], r[3]) for r in host_res]
    assert [_bits(d) for d in ctx.duals_lockstep()] == host and all(h is not None for h in host)


# ---- 4. the tall forms against the slack form -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1, 300, 40, 0), (1, 300, 40, 1), (1, 300, 40, 5), (1, 1100, 130, 17)],
                         ids=["300x40+0", "300x40+1", "300x40+5", "1100x130+17"])
def test_tall_forms_against_the_slack_form(ctx, case):
    """lpipm_upload_ub_tall (no `eq` rows) / lpipm_upload_ub_eq_tall against lpipm_upload_ub_eq on the same LP: the contract the
    header gives x -- the same status and count, the values to X_TOL."""
    prob = _problem(*planted_eq(*case)[:5])
    ctx.upload(prob)
    old = ctx.solve_raw(_opts())
    d_old = ctx.duals()
    ctx.upload_tall_eq(prob) if case[3] else ctx.upload(prob, tall=True)
    new = ctx.solve_raw(_opts())
    d_new = ctx.duals()
    assert old[0] == new[0] == OK and old[3] == new[3], (old[0], new[0], old[3], new[3])
    err = max(np.abs(d_new["y"] - d_old["y"]).max(), np.abs(d_new["z"] - d_old["z"]).max())
    print(f"\n[measure] tall vs slack form {case}: {new[3]} iterations, max|d duals| {err:.3g}")
    assert d_new["y"].shape == d_old["y"].shape and d_new["z"].shape == d_old["z"].shape and err <= X_TOL, err
    assert abs(d_new["dual_fun"] - d_old["dual_fun"]) <= 1e-6 * max(1.0, abs(d_old["dual_fun"]))


# ---- 5. scaling ---------------------------------------------------------------------------------------------------------------------
def _disturbed(A, b, c, seed):
    """The LP with its rows and columns taken by powers of two up to 2^+-16 (x_j -> x_j / dc_j: the same LP in other units)."""
    r = np.random.default_rng(900 + seed)
    kr, kc = r.integers(-16, 17, A.shape[0]), r.integers(-16, 17, A.shape[1])
    return np.ldexp(A, kr[:, None] + kc[None, :]), np.ldexp(b, kr), np.ldexp(c, kc)


def _host_scaled(A, b, c, kr, kc):
    return np.ldexp(A, kr[:, None].astype(np.int64) + kc[None, :]), np.ldexp(b, kr), np.ldexp(c, kc)


def _expect_unscaled(d, kr, kc):
    return dict(d, y=np.ldexp(d["y"], kr), z=np.ldexp(d["z"], -kc))


@pytest.fixture
def scaled_ctx(ctx):
    yield ctx
    ctx.set_scaling(0)


def test_scaled_single_lp(scaled_ctx):
    ctx = scaled_ctx
    from lp_amd import synth
    A0, b0, c0v, _ = synth.planted_lp(MEMBER_SEED, 24, 56)
    A, b, c = _disturbed(A0, b0, c0v, 0)
    ctx.set_scaling(8).upload_arrays(A, b, c)
    rc, x, fun, it, rows = ctx.solve_raw(_opts(), want_log=True)
    assert rc == OK
    d = ctx.duals()
    kr, kc = ctx.scaling()
    assert kr.any() and kc.any()
    As, bs_, cs_ = _host_scaled(A, b, c, kr, kc)
    ctx.set_scaling(0).upload_arrays(As, bs_, cs_)
    rc2, x2, fun2, it2, rows2 = ctx.solve_raw(_opts(), want_log=True)
    assert (rc2, it2) == (rc, it) and rows2 == rows
    want = _expect_unscaled(ctx.duals(), kr, kc)
    assert _bits(d) == _bits(want)
    # identity 1 against the caller's A, b, c; rho_d and the norm are the scaled problem's
    check_identities(A, b, c, 0.0, x, fun, d, rows[-1][:3] + (None, rows[-1][4], None, rows[-1][6]), "scaled 24x56",
                     norm_c=max(1.0, np.linalg.norm(cs_ - 1.0)), col_exp=kc)


@pytest.mark.parametrize("own", [False, True], ids=["shared: one exponent set", "own matrices: one set per member"])
def test_scaled_batches(scaled_ctx, own):
    from lp_amd import synth
    ctx = scaled_ctx
    K = 4
    if own:
        mem = [_disturbed(*dense_own_member(k), k) for k in range(K)]
        ctx.set_scaling(8).upload_lockstep([q[0] for q in mem], [q[1] for q in mem], [q[2] for q in mem])
    else:
        A0, bs0, cs0 = _dense_shared()
        r = np.random.default_rng(901)
        kr0, kc0 = r.integers(-16, 17, 24), r.integers(-16, 17, 56)
        mem = [(np.ldexp(A0, kr0[:, None] + kc0[None, :]), np.ldexp(bs0[k], kr0), np.ldexp(cs0[k], kc0)) for k in range(K)]
        ctx.set_scaling(8).upload_lockstep_shared(mem[0][0], [q[1] for q in mem], [q[2] for q in mem])
    res = ctx.solve_lockstep(_opts())
    assert all(r_[0] == OK for r_ in res)
    got = ctx.duals_lockstep()
    exps = [ctx.scaling(k if own else 0) for k in range(K)]
    if own:
        assert any((exps[0][1] != exps[k][1]).any() for k in range(1, K))      # really one set per member
    ctx.set_scaling(0)
    for k in range(K):
        kr, kc = exps[k]
        As, bs_, cs_ = _host_scaled(*mem[k], kr, kc)
        ctx.upload_arrays(As, bs_, cs_)
        rc, x, fun, it, rows = ctx.solve_raw(_opts(), want_log=True)
        assert (rc, it) == (res[k][0], res[k][3])
        assert _bits(got[k]) == _bits(_expect_unscaled(ctx.duals(), kr, kc)), k
        # identity 1 against the member's own (disturbed) A, b, c and the batch's x and duals; rho_d and the norm are the scaled
        # problem's, which this bit-identical solve of the host-scaled LP logs (a lockstep solve keeps no log)
        check_identities(*mem[k], 0.0, res[k][1], res[k][2], got[k], rows[-1][:3] + (None, rows[-1][4], None, rows[-1][6]),
                         f"scaled batch member {k} own={own}", norm_c=max(1.0, np.linalg.norm(cs_ - 1.0)), col_exp=kc)


# ---- 6. validity and refusals -------------------------------------------------------------------------------------------------------
def test_validity_and_refusals():
    import lp_amd
    import torch
    from lp_amd import _capi, synth
    lib = _capi.lib()
    cx = lp_amd.Context(0)
    try:
        A, b, c, _ = synth.planted_lp(MEMBER_SEED, 24, 56)
        m, n = A.shape
        get = lambda member=0: _raw_get(cx, member, m, n)[0]
        assert get() == NO_PROBLEM                               # before any upload
        cx.upload_arrays(A, b, c)
        assert get() == NO_PROBLEM                               # before any solve
        assert cx.solve_raw(_opts())[0] == OK
        assert get() == OK
        assert get(1) == BAD_ARGUMENT and get(2 ** 40) == BAD_ARGUMENT      # a member that is not there
        assert get() == OK
        cx.update_vectors(b, c)
        assert get() == NO_PROBLEM                               # b and c are new, the iterate is old
        assert cx.solve_raw(_opts())[0] == OK and get() == OK
        cx.k_iteration(_opts(), np.ones(n), np.zeros(m), np.ones(n), 1.0, 1.0, ip=True)
        assert get() == NO_PROBLEM                               # a kernel entry wrote the iterate
        assert cx.solve_raw(_opts())[0] == OK and get() == OK
        cx.upload_arrays(A, b, c)
        assert get() == NO_PROBLEM                               # a new upload
        # the QR arms leave the same iterate
        assert cx.solve_raw(_opts())[0] == OK
        chol = cx.duals()
        for arm in (1, 2):
            assert cx.solve_raw(_opts(solver_type=arm))[0] == OK
            d = cx.duals()
            err = max(np.abs(d["y"] - chol["y"]).max(), np.abs(d["z"] - chol["z"]).max())
            print(f"\n[measure] solver_type {arm}: max|d duals| against the Cholesky arm {err:.3g}")
            assert err <= X_TOL
        # a lockstep batch: update_lockstep_vectors invalidates; the device entry's refusals
        As, bs, cs = _dense_shared()
        K = 3
        cx.upload_lockstep_shared(As, bs[:K], cs[:K])
        assert get() == NO_PROBLEM
        assert all(r[0] == OK for r in cx.solve_lockstep(_opts()))
        assert get(K - 1) == OK and get(K) == BAD_ARGUMENT
        yd = torch.full((K, m), -7.0, dtype=torch.float64, device="cuda")
        zd = torch.full((K, n), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        dev = lambda yp, ldy, zp, ldz: lib.lpipm_get_duals_device(cx._h, C.c_void_p(yp) if yp else None, ldy,
                                                                  C.c_void_p(zp) if zp else None, ldz, None)
        assert dev(yd.data_ptr(), m, zd.data_ptr(), n) == OK
        assert dev(yd.data_ptr(), m - 1, zd.data_ptr(), n) == BAD_ARGUMENT           # ldy too small
        assert dev(yd.data_ptr(), m, zd.data_ptr(), n - 1) == BAD_ARGUMENT           # ldz too small
        # rows that would end outside the allocation (far outside: torch's allocator hands out parts of larger blocks)
        assert dev(yd.data_ptr(), 1 << 40, zd.data_ptr(), n) == BAD_ARGUMENT
        assert (yd.cpu().numpy()[:, 0] != -7.0).all()                                # (the first call delivered)
        host = np.zeros((K, m))
        assert dev(host.ctypes.data, m, zd.data_ptr(), n) == BAD_ARGUMENT            # a host pointer
        assert dev(None, 0, None, 0) == OK                                           # nothing asked for: the infos alone
        cx.update_lockstep_vectors(bs[:K], cs[:K])
        assert get() == NO_PROBLEM and dev(yd.data_ptr(), m, zd.data_ptr(), n) == NO_PROBLEM
        assert all(r[0] == OK for r in cx.solve_lockstep(_opts())) and get() == OK
        # a solve that returns a runtime code leaves no duals either (the QR arms are single-LP: LPIPM_ERR_UNSUPPORTED)
        with pytest.raises(lp_amd.BackendError):
            cx.solve_lockstep(_opts(solver_type=1))
        assert get() == NO_PROBLEM
    finally:
        cx.close()


def _batch_entries():
    """(name, call(cx) -> results) for the four lpipm_solve_batch* entries, each over members of two shapes: three of one
    shape (a lockstep chunk on the context) and one odd one (solved one at a time)."""
    import torch
    dense = [dense_own_member(k) + (0.0,) for k in range(3)] + [tuple(case_arrays(("planted", 48, 96))[k] for k in "Abc") + (0.0,)]
    slack = [slack_form(*_parts(SLACK_MEMBER, True, k)) + (0.0, SLACK_MEMBER[0]) for k in range(3)] + \
            [slack_form(*planted_eq(1, 40, 8, 2)[:5]) + (0.0, 40)]
    tall = [_problem(*_parts(TALL_MEMBER, True, k)) for k in range(3)] + [_problem(*planted_eq(1, 40, 8, 0)[:5])]

    def device(cx):
        x = torch.zeros((4, 96), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        return cx.solve_batch_device(dense, _opts(), x.data_ptr(), 96)
    return [("lpipm_solve_batch", lambda cx: cx.solve_batch(dense, _opts())), ("lpipm_solve_batch_device", device),
            ("lpipm_solve_batch_slack", lambda cx: cx.solve_batch(slack, _opts())),
            ("lpipm_solve_batch_ub_tall", lambda cx: cx.solve_batch(tall, _opts(), tall=True))]


@pytest.mark.parametrize("which", range(4), ids=["solve_batch", "solve_batch_device", "solve_batch_slack", "solve_batch_ub_tall"])
def test_no_duals_after_a_batch_solve(which):
    """lpipm_solve_batch* replace the resident problem chunk by chunk and member by member, on the context itself: whatever
    they leave resident is not the caller's, and both getter entries say LPIPM_ERR_NO_PROBLEM -- whether or not the context
    had duals before, with and without lockstep chunks."""
    import lp_amd
    from lp_amd import _capi
    name, call = _batch_entries()[which]
    cx = lp_amd.Context(0)
    try:
        a = case_arrays(("planted", 24, 56))
        for max_group in (-1, 0):
            cx.upload_arrays(a["A"], a["b"], a["c"])
            assert cx.solve_raw(_opts())[0] == OK and _raw_get(cx, 0, 24, 56)[0] == OK
            _capi.lib().lpipm_set_batch_lockstep(cx._h, max_group)
            res = call(cx)
            assert len(res) == 4 and all(r[0] == OK for r in res), (name, [r[0] for r in res])
            rc, y, z, info = _raw_get(cx, 0, 4096, 4096)                    # (buffers larger than any member's vectors)
            assert rc == NO_PROBLEM and (y == -7.0).all() and (z == -7.0).all() and info.status == -7, (name, max_group, rc)
            assert _capi.lib().lpipm_get_duals_device(cx._h, None, 0, None, 0, None) == NO_PROBLEM, (name, max_group)
            with pytest.raises(lp_amd.BackendError):
                cx.duals()
            with pytest.raises(lp_amd.BackendError):
                cx.duals_lockstep()
            with pytest.raises(lp_amd.BackendError):
                cx.duals_device(None, 0, None, 0)
    finally:
        cx.close()


# ---- 7. the getter leaves nothing behind ------------------------------------------------------------------------------------------
def _solve_get_solve(upload, batch):
    """On a fresh context: solve, get the duals by both entries, solve again.  -> (first, second, resident bytes)."""
    import lp_amd
    import torch
    cx = lp_amd.Context(0)
    try:
        upload(cx)
        run = (lambda: [(r[0], r[1].tobytes(), r[2], r[3]) for r in cx.solve_lockstep(_opts())]) if batch else \
              (lambda: (lambda r: (r[0], r[1].tobytes(), r[2], r[3], tuple(r[4])))(cx.solve_raw(_opts(), want_log=True)))
        first = run()
        K = cx._members
        for k in range(K):
            cx.duals(k)
        yd = torch.empty((K, cx.m), dtype=torch.float64, device="cuda")
        zd = torch.empty((K, cx.n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        cx.duals_device(yd.data_ptr(), cx.m, zd.data_ptr(), cx.n)
        return first, run(), cx.resident_bytes()
    finally:
        cx.close()


def _fresh(upload, batch):
    import lp_amd
    cx = lp_amd.Context(0)
    try:
        upload(cx)
        if batch:
            return [(r[0], r[1].tobytes(), r[2], r[3]) for r in cx.solve_lockstep(_opts())], cx.resident_bytes()
        r = cx.solve_raw(_opts(), want_log=True)
        return (r[0], r[1].tobytes(), r[2], r[3], tuple(r[4])), cx.resident_bytes()
    finally:
        cx.close()


@pytest.mark.parametrize("which", ["130x300", "tall-eq 300x40+5", "batch of 16"])
def test_the_getter_leaves_nothing_behind(which):
    if which == "130x300":
        a = case_arrays(("planted", 130, 300))
        upload, batch = (lambda cx: cx.upload_arrays(a["A"], a["b"], a["c"])), False
    elif which.startswith("tall-eq"):
        prob = _problem(*planted_eq(1, 300, 40, 5)[:5])
        upload, batch = (lambda cx: cx.upload_tall_eq(prob)), False
    else:
        A, bs, cs = _dense_shared()
        upload, batch = (lambda cx: cx.upload_lockstep_shared(A, bs[:16], cs[:16])), True
    first, second, nbytes = _solve_get_solve(upload, batch)
    fresh, fresh_bytes = _fresh(upload, batch)
    assert second == first, which           # x, fun, count (and the log of a single LP), bit for bit
    assert first == fresh and nbytes == fresh_bytes, which


# ---- 8. the Python drivers ----------------------------------------------------------------------------------------------------------
def test_python_drivers(ctx):
    import lp_amd
    from lp_amd import batch
    A, bs, cs = _dense_shared()
    bs, cs = bs[:7], cs[:7]
    plain = batch.solve_shared_matrix(A, bs, cs, ctx=ctx, max_group=3)
    swept = batch.sweep_shared_matrix(A, bs, cs, ctx=ctx, max_group=3)
    for out in (plain, swept):
        assert all(set(q) == {"status", "x_slack", "fun", "iterations"} for q in out)         # exactly today's dicts
    a = batch.solve_shared_matrix(A, bs, cs, ctx=ctx, max_group=3, duals=True)
    b = batch.sweep_shared_matrix(A, bs, cs, ctx=ctx, max_group=3, duals=True)
    assert len(a) == len(b) == 7
    for k, (p, q, r) in enumerate(zip(a, b, plain)):
        assert set(p) == set(q) == {"status", "x_slack", "fun", "iterations", "y", "z", "dual_fun"}
        assert p["status"] == q["status"] == OK and p["iterations"] == q["iterations"]
        for key in ("x_slack", "y", "z", "fun", "dual_fun"):
            assert np.asarray(p[key]).tobytes() == np.asarray(q[key]).tobytes(), (k, key)
        assert p["x_slack"].tobytes() == r["x_slack"].tobytes() and p["fun"] == r["fun"]
        assert _bits(dict(p, tau=0.0, kappa=0.0))[:3] == _single_result(ctx, "shared", k)[2][:3]
    # the solver front end
    X, b_, Ae, be, c, _ = planted_eq(1, 40, 8, 2)
    prob = _problem(X, b_, Ae, be, c)
    solver = lp_amd.InteriorPoint.default()
    res = solver.solve_with_duals(prob)
    base = solver.solve(prob)
    assert res.x().tobytes() == base.x().tobytes() and res.fun() == base.fun() and res.iteration() == base.iteration()
    assert res.y_ub.shape == (40,) and res.y_eq.shape == (2,) and res.reduced_costs.shape == (8,)
    assert (res.y_ub <= X_TOL).all() and (res.reduced_costs > 0).all()       # (a `ub` multiplier is <= 0 up to the dual residual)
    assert np.abs(c - X.T @ res.y_ub - Ae.T @ res.y_eq - res.reduced_costs).max() <= X_TOL
    assert abs(res.dual_fun - res.fun()) <= 1e-6 * max(1.0, abs(res.fun()))
    assert not hasattr(base, "y_ub")


def test_solve_device_with_duals(ctx):
    import torch
    from lp_amd import batch
    A, bs, cs = _dense_shared()
    K = 5
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    x, st, fun, its, y, z, dual_fun = batch.solve_device(t(A), t(np.stack(bs[:K])), t(np.stack(cs[:K])), ctx=ctx, max_group=3,
                                                         duals=True)
    assert len(batch.solve_device(t(A), t(np.stack(bs[:K])), t(np.stack(cs[:K])), ctx=ctx, max_group=3)) == 4
    yh, zh = y.cpu().numpy(), z.cpu().numpy()
    for k in range(K):
        want = _single_result(ctx, "shared", k)[2]
        assert st[k] == OK and (yh[k].tobytes(), zh[k].tobytes(), np.float64(dual_fun[k]).tobytes()) == want[:3], k
