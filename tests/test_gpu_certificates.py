"""Infeasibility and unboundedness certificates of the last solve (lpipm_get_certificate, lpipm_get_certificate_device; DESIGN
3.12.1) on the device: parity with the oracle's certificate, the numpy checks against the caller's own arrays, bit-identity of
every member across every resident form, count and entry, scaling, a getter that leaves nothing behind, validity and refusals,
the Python drivers.  Inputs, oracle construction and numpy checks: tests/test_certificates_host.py."""
import ctypes as C

import numpy as np
import pytest

from test_certificates_host import (CASES, FARKAS, IDS, NONE, RAY, X_TOL, batch_member, case_lp, check_certificate,
                                    check_ray_identities, limit_for, oracle_pair, role, want_status)
from test_tall_eq_host import slack_form

pytestmark = pytest.mark.gpu

OK, INFEASIBLE, UNBOUNDED, ITERATION_LIMIT = 0, 5, 6, 7
NO_PROBLEM, UNSUPPORTED, BAD_ARGUMENT = 101, 102, 103
SENTINEL = -7.0


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _has_x(rc):
    return rc in (OK, ITERATION_LIMIT)


def _problem(X, b, Ae, be, c):
    import lp_amd
    p = lp_amd.Problem.target(c).ub(X, b)
    return (p.eq(Ae, be) if Ae.shape[0] else p).build()


def _f64(v):
    return np.float64(v).tobytes()


def _bits(d):
    """A certificate dict as bytes: kind, status, the vectors (None stays None), scale, residual, tau, kappa."""
    vec = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()
    return (d["kind"], d["status"], vec(d["y"]), vec(d["col"]), _f64(d["scale"]), _f64(d["residual"]), _f64(d["tau"]), _f64(d["kappa"]))


def _info_bits(r):
    return (int(r.kind), int(r.status), _f64(r.scale), _f64(r.residual), _f64(r.tau), _f64(r.kappa))


def _raw_get(cx, member, m, n, info=True):
    """lpipm_get_certificate itself: -> (rc, y, col, info) with sentinel-filled outputs."""
    from lp_amd import _capi
    y, col = np.full(m, SENTINEL), np.full(n, SENTINEL)
    rec = _capi.CertInfo(SENTINEL, SENTINEL, SENTINEL, SENTINEL, -7, -7)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = _capi.lib().lpipm_get_certificate(cx._h, member, dp(y), dp(col), C.byref(rec) if info else None)
    return rc, y, col, rec


def _duals_bits(cx, member=0):
    import lp_amd
    try:
        d = cx.duals(member)
    except lp_amd.LinearProgramError:
        return None
    return tuple(np.ascontiguousarray(d[k], dtype=np.float64).tobytes() for k in ("y", "z", "dual_fun", "tau", "kappa"))


def _upload_case(cx, case, k=0):
    form = case[0]
    d = case_lp(case, k)
    if form == "dense":
        return cx.upload_arrays(d["A"], d["b"], d["c"])
    prob = _problem(*d["parts"])
    if form == "slack":
        return cx.upload(prob)
    return cx.upload_tall_eq(prob) if form == "tall_eq" else cx.upload(prob, tall=True)


# ---- 1 and 2. the oracle, and the caller's own arrays -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_certificates_match_the_oracle_and_the_callers_arrays(ctx, case):
    d = case_lp(case)
    ref, alt = oracle_pair(case)
    _upload_case(ctx, case)
    rc, x, fun, it, rows = ctx.solve_raw(_opts(), want_log=True)
    cert = ctx.certificate()
    assert rc == cert["status"] == ref["status"] == alt["status"] == want_status(case), (rc, ref["status"])
    assert it in (ref["iterations"], alt["iterations"]) and len(rows) == it, (it, ref["iterations"], alt["iterations"])
    assert cert["kind"] == ref["kind"] == (FARKAS if rc == INFEASIBLE else RAY)
    assert cert["col"].shape == d["c"].shape and (cert["y"] is None) == (cert["kind"] == RAY)
    worst = 0.0
    for got, key in ((cert["y"], "yh"), (cert["col"], "col")):
        if got is None:
            continue
        assert got.shape == ref[key].shape
        lo, hi = np.minimum(ref[key], alt[key]), np.maximum(ref[key], alt[key])
        worst = max(worst, np.maximum(np.maximum(lo - got, got - hi), 0.0).max())
    print(f"\n[measure] {case}: {it} iterations, ray outside the oracle's envelope by {worst:.3g}, scale {cert['scale']:.6g} "
          f"(the oracle's {ref['scale']:.6g})")
    assert worst <= X_TOL, worst
    assert cert["scale"] > 0 and cert["tau"] > 0
    check_certificate(d["A"], d["b"], d["c"], cert, f"gpu {case}")
    check_ray_identities(d["A"], d["b"], d["c"], cert, rows[-1], f"gpu {case}")


# ---- 3. bit-identity across paths ---------------------------------------------------------------------------------------------------
# form -> (the kind of its members, upload of the members as one batch, upload of one member alone)
def _form(name):
    kind = {"lockstep": "dense-own", "shared": "dense", "lockstep_slack": "slack-own", "shared_slack": "slack",
            "shared_ub_eq": "slack", "shared_ub_tall": "tall", "shared_ub_eq_tall": "tall-eq", "lockstep_ub_tall": "tall-own"}[name]
    if name in ("lockstep", "shared"):
        single = lambda cx, mem: cx.upload_arrays(*mem)
        if name == "lockstep":
            return kind, (lambda cx, mems: cx.upload_lockstep(*map(list, zip(*mems)))), single
        return kind, (lambda cx, mems: cx.upload_lockstep_shared(mems[0][0], [q[1] for q in mems], [q[2] for q in mems])), single
    if name in ("lockstep_slack", "shared_slack"):
        ns = lambda mem: mem[0].shape[0]
        single = lambda cx, mem: cx.upload_arrays(*slack_form(*mem), 0.0, ns(mem))
        if name == "lockstep_slack":
            return kind, (lambda cx, mems: cx.upload_lockstep(*map(list, zip(*[slack_form(*q) for q in mems])), n_slack=ns(mems[0]))), single
        return kind, (lambda cx, mems: cx.upload_lockstep_shared(slack_form(*mems[0])[0], [slack_form(*q)[1] for q in mems],
                                                                 [slack_form(*q)[2] for q in mems], n_slack=ns(mems[0]))), single
    tall = name != "shared_ub_eq"

    def single(cx, mem):
        prob = _problem(*mem)
        if not tall:
            return cx.upload(prob)
        return cx.upload_tall_eq(prob) if mem[2].shape[0] else cx.upload(prob, tall=True)

    def batch(cx, mems):
        X, _, Ae, _, _ = mems[0]
        bs, cs = [np.concatenate([q[1], q[3]]) for q in mems], [q[4] for q in mems]
        if name == "shared_ub_eq":
            return cx.upload_lockstep_shared_ub_eq(X, Ae, bs, cs)
        if name == "shared_ub_tall":
            return cx.upload_lockstep_shared_ub_tall(X, bs, cs)
        if name == "shared_ub_eq_tall":
            return cx.upload_lockstep_shared_ub_eq_tall(X, Ae, bs, cs)
        return cx.upload_lockstep_ub_tall([q[0] for q in mems], bs, cs)
    return kind, batch, single


FORMS = ["lockstep", "lockstep_slack", "shared", "shared_slack", "shared_ub_eq", "shared_ub_tall", "shared_ub_eq_tall",
         "lockstep_ub_tall"]
_singles = {}


def _single_result(ctx, name, k, which, **okw):
    """Member k of the form alone in the role `which`: upload + lpipm_solve + lpipm_get_duals (where it has a solution) +
    lpipm_get_certificate.  Computed once per (form, member, role, options).  -> (rc, iterations, duals, certificate) as bytes"""
    key = (name, k, which, tuple(sorted(okw.items())))
    if key not in _singles:
        kind, _, single = _form(name)
        single(ctx, batch_member(kind, k, which))
        rc, x, fun, it, _ = ctx.solve_raw(_opts(**okw))
        duals = _duals_bits(ctx)                                   # the duals first here, the certificate first in the batch
        _singles[key] = (rc, it, duals, _bits(ctx.certificate()))
    return _singles[key]


@pytest.mark.parametrize("K", [3, 16, 18])
@pytest.mark.parametrize("name", FORMS)
def test_every_member_has_the_bits_of_its_single_solve(ctx, name, K):
    """An infeasible member at position 1, an unbounded one last; the iteration limit is the unbounded member's count, which
    (16 and 18 members) leaves good members finished and good members at the limit."""
    import torch
    from lp_amd import _capi
    kind, batch, _ = _form(name)
    mems = [batch_member(kind, k, role(k, K)) for k in range(K)]
    batch(ctx, mems)
    free = ctx.solve_lockstep(_opts())
    want = [{"infeasible": INFEASIBLE, "unbounded": UNBOUNDED, "good": OK}[role(k, K)] for k in range(K)]
    assert [r[0] for r in free] == want, (name, K, [r[0] for r in free])
    L = limit_for([(r[0], r[3]) for r in free])
    batch(ctx, mems)
    res = ctx.solve_lockstep(_opts(max_iter=L))
    codes = [r[0] for r in res]
    assert codes[1] == INFEASIBLE and codes[-1] == UNBOUNDED and all(_has_x(c) for k, c in enumerate(codes) if role(k, K) == "good")
    assert K == 3 or (OK in codes and ITERATION_LIMIT in codes), (name, K, L, codes)
    got = ctx.certificates_lockstep()                              # the device entry: one call, one copy
    m, n = ctx.m, ctx.n
    # the device entry into rows wider than the vectors, pre-filled: gaps and the rows of members without a certificate stay
    ldy, ldc = m + 3, n + 5
    yd = torch.full((K, ldy), SENTINEL, dtype=torch.float64, device="cuda")
    cd = torch.full((K, ldc), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    info = (_capi.CertInfo * K)()
    assert _capi.lib().lpipm_get_certificate_device(ctx._h, C.c_void_p(yd.data_ptr()), ldy, C.c_void_p(cd.data_ptr()), ldc, info) == OK
    yh, ch = yd.cpu().numpy(), cd.cpu().numpy()
    assert (yh[:, m:] == SENTINEL).all() and (ch[:, n:] == SENTINEL).all()
    host = [ctx.certificate(k) for k in range(K)]                  # the host entry, member by member
    duals = [_duals_bits(ctx, k) for k in range(K)]                # lpipm_get_duals after the getter, on the same context
    for k in range(K):
        rc1, it1, duals1, cert1 = _single_result(ctx, name, k, role(k, K), max_iter=L)
        assert (res[k][0], res[k][3]) == (rc1, it1), (name, K, k)
        assert _bits(got[k]) == cert1 and _bits(host[k]) == cert1, (name, K, k)
        assert _info_bits(info[k]) == cert1[:2] + cert1[4:], (name, K, k)
        assert duals[k] == duals1 and (duals1 is not None) == _has_x(rc1), (name, K, k)
        kind_k = got[k]["kind"]
        assert kind_k == {INFEASIBLE: FARKAS, UNBOUNDED: RAY}.get(rc1, NONE) and got[k]["status"] == rc1
        if kind_k == NONE:
            assert (yh[k] == SENTINEL).all() and (ch[k] == SENTINEL).all() and got[k]["y"] is None and got[k]["col"] is None
            assert np.isnan(got[k]["scale"]) and np.isnan(got[k]["residual"]) and got[k]["tau"] > 0
        else:
            assert ch[k, :n].tobytes() == got[k]["col"].tobytes()
            assert (yh[k, :m].tobytes() == got[k]["y"].tobytes()) if kind_k == FARKAS else (yh[k] == SENTINEL).all()


def test_upload_device_gives_the_bits_of_its_host_entry(ctx):
    import torch
    K = 5
    mems = [slack_form(*batch_member("slack", k, role(k, K))) for k in range(K)]
    A, bs, cs = mems[0][0], [q[1] for q in mems], [q[2] for q in mems]
    ns = A.shape[0] - 8
    ctx.upload_lockstep_shared(A, bs, cs, n_slack=ns)
    host_res = ctx.solve_lockstep(_opts())
    host = [_bits(d) for d in ctx.certificates_lockstep()]
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64, device="cuda")
    ctx.upload_device(t(A), t(np.stack(bs)), t(np.stack(cs)), n_slack=ns)
    dev_res = ctx.solve_lockstep(_opts())
    assert [(r[0], r[3]) for r in dev_res] == [(r[0], r[3]) for r in host_res]
    assert [r[0] for r in host_res] == [OK, INFEASIBLE, OK, OK, UNBOUNDED]
    assert [_bits(d) for d in ctx.certificates_lockstep()] == host and [h[0] for h in host] == [NONE, FARKAS, NONE, NONE, RAY]


# ---- 4. scaling ---------------------------------------------------------------------------------------------------------------------
def _disturbed(A, b, c, seed):
    """The LP with its rows and columns taken by powers of two up to 2^+-16 (the helper of tests/test_gpu_scaling.py)."""
    r = np.random.default_rng(900 + seed)
    kr, kc = r.integers(-16, 17, A.shape[0]), r.integers(-16, 17, A.shape[1])
    return np.ldexp(A, kr[:, None] + kc[None, :]), np.ldexp(b, kr), np.ldexp(c, kc)


def _host_scaled(A, b, c, kr, kc):
    return np.ldexp(A, kr[:, None].astype(np.int64) + kc[None, :]), np.ldexp(b, kr), np.ldexp(c, kc)


def _expect_unscaled(d, kr, kc):
    """The certificate of the host-scaled LP in the caller's units: y^ by kr, z^ by -kc, x^ by kc."""
    if d["kind"] == FARKAS:
        return dict(d, y=np.ldexp(d["y"], kr), col=np.ldexp(d["col"], -kc))
    return dict(d, col=np.ldexp(d["col"], kc)) if d["kind"] == RAY else d


def _but_residual(bits):
    """(the residual is in the caller's units: that of the host-scaled LP is in its own)"""
    return bits[:5] + bits[6:]


@pytest.fixture
def scaled_ctx(ctx):
    yield ctx
    ctx.set_scaling(0)


@pytest.mark.parametrize("which", ["infeasible", "unbounded"])
def test_scaled_single_lp(scaled_ctx, which):
    ctx = scaled_ctx
    d0 = case_lp(("dense", (24, 56), which))
    A, b, c = _disturbed(d0["A"], d0["b"], d0["c"], 0)
    ctx.set_scaling(8).upload_arrays(A, b, c)
    rc, x, fun, it, rows = ctx.solve_raw(_opts(), want_log=True)
    assert rc == want_status((None, None, which))
    cert = ctx.certificate()
    kr, kc = ctx.scaling()
    assert kr.any() and kc.any()
    As, bs_, cs_ = _host_scaled(A, b, c, kr, kc)
    ctx.set_scaling(0).upload_arrays(As, bs_, cs_)
    rc2, x2, fun2, it2, rows2 = ctx.solve_raw(_opts(), want_log=True)
    assert (rc2, it2) == (rc, it) and rows2 == rows
    want = _expect_unscaled(ctx.certificate(), kr, kc)
    assert _but_residual(_bits(cert)) == _but_residual(_bits(want)) and cert["kind"] != NONE
    # in the caller's units, against the caller's A, b, c; rho_p, rho_d and the norms are the scaled problem's
    check_certificate(A, b, c, cert, f"scaled 25x56 {which}")
    check_ray_identities(A, b, c, cert, rows[-1], f"scaled 25x56 {which}", norm_b=max(1.0, np.linalg.norm(bs_ - As @ np.ones(As.shape[1]))),
                         norm_c=max(1.0, np.linalg.norm(cs_ - 1.0)), row_exp=kr, col_exp=kc)


@pytest.mark.parametrize("own", [False, True], ids=["shared: one exponent set", "own matrices: one set per member"])
def test_scaled_batches(scaled_ctx, own):
    ctx = scaled_ctx
    K = 4
    if own:
        mem = [_disturbed(*_dense_case(k, K), k) for k in range(K)]
        ctx.set_scaling(8).upload_lockstep([q[0] for q in mem], [q[1] for q in mem], [q[2] for q in mem])
    else:
        base = [slack_form(*batch_member("slack", k, role(k, K))) for k in range(K)]
        r = np.random.default_rng(901)
        kr0, kc0 = r.integers(-16, 17, base[0][0].shape[0]), r.integers(-16, 17, base[0][0].shape[1])
        mem = [(np.ldexp(q[0], kr0[:, None] + kc0[None, :]), np.ldexp(q[1], kr0), np.ldexp(q[2], kc0)) for q in base]
        ctx.set_scaling(8).upload_lockstep_shared(mem[0][0], [q[1] for q in mem], [q[2] for q in mem])
    res = ctx.solve_lockstep(_opts())
    assert [r_[0] for r_ in res] == [OK, INFEASIBLE, OK, UNBOUNDED]
    got = ctx.certificates_lockstep()
    exps = [ctx.scaling(k if own else 0) for k in range(K)]
    if own:
        assert any((exps[0][1] != exps[k][1]).any() for k in range(1, K))      # really one set per member
    ctx.set_scaling(0)
    for k in range(K):
        kr, kc = exps[k]
        ctx.upload_arrays(*_host_scaled(*mem[k], kr, kc))
        rc, x, fun, it, _ = ctx.solve_raw(_opts())
        assert (rc, it) == (res[k][0], res[k][3])
        assert _but_residual(_bits(got[k])) == _but_residual(_bits(_expect_unscaled(ctx.certificate(), kr, kc))), k
        if got[k]["kind"] != NONE:
            check_certificate(*mem[k], got[k], f"scaled batch member {k} own={own}")
    assert [g["kind"] for g in got] == [NONE, FARKAS, NONE, RAY]


def _dense_case(k, K):
    """Member k of the own-matrix dense batch of the scaling test: the 25 x 56 LPs of the parity cases, each with its own matrix."""
    d = case_lp(("dense", (24, 56), role(k, K)), k)
    return d["A"], d["b"], d["c"]


# ---- 5. nothing left behind -----------------------------------------------------------------------------------------------------------
def _run(cx, batch):
    if batch:
        return [(r[0], None if r[1] is None else r[1].tobytes(), r[2], r[3]) for r in cx.solve_lockstep(_opts())]
    r = cx.solve_raw(_opts(), want_log=True)
    return (r[0], None if r[1] is None else r[1].tobytes(), _f64(r[2]), r[3], tuple(r[4]))


def _solve_get_solve(upload, batch):
    """On a fresh context: solve, the certificates by both entries, lpipm_get_duals of the members that have a solution, solve
    again.  -> (first, second, resident bytes, kinds)"""
    import lp_amd
    import torch
    cx = lp_amd.Context(0)
    try:
        upload(cx)
        first = _run(cx, batch)
        K = cx._members
        kinds = [cx.certificate(k)["kind"] for k in range(K)]
        yd = torch.empty((K, cx.m), dtype=torch.float64, device="cuda")
        cd = torch.empty((K, cx.n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        cx.certificates_device(yd.data_ptr(), cx.m, cd.data_ptr(), cx.n)
        codes = [r[0] for r in first] if batch else [first[0]]
        for k in range(K):
            if _has_x(codes[k]):
                cx.duals(k)
        return first, _run(cx, batch), cx.resident_bytes(), kinds
    finally:
        cx.close()


def _fresh(upload, batch):
    import lp_amd
    cx = lp_amd.Context(0)
    try:
        upload(cx)
        return _run(cx, batch), cx.resident_bytes()
    finally:
        cx.close()


@pytest.mark.parametrize("which", ["131x300 infeasible", "131x300 unbounded", "tall-eq 300x40+5 infeasible",
                                   "tall-eq 300x40+5 unbounded", "batch of 16"])
def test_the_getter_leaves_nothing_behind(which):
    if which.startswith("131x300"):
        a = case_lp(("dense", (130, 300), which.split()[1]))
        upload, batch = (lambda cx: cx.upload_arrays(a["A"], a["b"], a["c"])), False
    elif which.startswith("tall-eq"):
        prob = _problem(*case_lp(("tall_eq", (300, 40, 5), which.split()[2]))["parts"])
        upload, batch = (lambda cx: cx.upload_tall_eq(prob)), False
    else:
        mems = [batch_member("dense", k, role(k, 16)) for k in range(16)]
        upload, batch = (lambda cx: cx.upload_lockstep_shared(mems[0][0], [q[1] for q in mems], [q[2] for q in mems])), True
    first, second, nbytes, kinds = _solve_get_solve(upload, batch)
    fresh, fresh_bytes = _fresh(upload, batch)
    assert FARKAS in kinds or RAY in kinds, kinds            # the getter's launches did run
    assert second == first, which           # status, x, fun, count (and the log of a single LP), bit for bit
    assert first == fresh and nbytes == fresh_bytes, which


# ---- 6. validity and refusals -------------------------------------------------------------------------------------------------------
def test_validity_and_refusals():
    import lp_amd
    import torch
    from lp_amd import _capi
    lib = _capi.lib()
    cx = lp_amd.Context(0)
    try:
        a = case_lp(("dense", (24, 56), "infeasible"))
        A, b, c = a["A"], a["b"], a["c"]
        m, n = A.shape
        get = lambda member=0: _raw_get(cx, member, m, n)[0]
        assert get() == NO_PROBLEM                               # before any upload
        cx.upload_arrays(A, b, c)
        assert get() == NO_PROBLEM                               # before any solve
        assert cx.solve_raw(_opts())[0] == INFEASIBLE
        rc, y, col, info = _raw_get(cx, 0, m, n)
        assert rc == OK and info.kind == FARKAS and info.status == INFEASIBLE and (y != SENTINEL).all() and (col != SENTINEL).all()
        assert get(1) == BAD_ARGUMENT and get(2 ** 40) == BAD_ARGUMENT      # a member that is not there
        rc, y, col, info = _raw_get(cx, 0, m, n, info=False)                 # a null info_out
        assert rc == BAD_ARGUMENT and (y == SENTINEL).all() and (col == SENTINEL).all()
        assert get() == OK
        cx.update_vectors(b, c)
        assert get() == NO_PROBLEM                               # b and c are new, the iterate is old
        assert cx.solve_raw(_opts())[0] == INFEASIBLE and get() == OK
        cx.k_iteration(_opts(), np.ones(n), np.zeros(m), np.ones(n), 1.0, 1.0, ip=True)
        assert get() == NO_PROBLEM                               # a kernel entry wrote the iterate
        assert cx.solve_raw(_opts())[0] == INFEASIBLE and get() == OK
        cx.upload_arrays(A, b, c)
        assert get() == NO_PROBLEM                               # a new upload
        # the QR arms leave the same ray
        assert cx.solve_raw(_opts())[0] == INFEASIBLE
        chol = cx.certificate()
        for arm in (1, 2):
            assert cx.solve_raw(_opts(solver_type=arm))[0] == INFEASIBLE
            d = cx.certificate()
            err = max(np.abs(d["y"] - chol["y"]).max(), np.abs(d["col"] - chol["col"]).max())
            print(f"\n[measure] solver_type {arm}: max|d ray| against the Cholesky arm {err:.3g}")
            assert d["kind"] == FARKAS and err <= X_TOL
        # a member with a solution: kind NONE, nothing written, scale and residual NaN, the iterate's tau and kappa
        g = case_lp(("dense", (24, 56), "good"))
        cx.upload_arrays(g["A"], g["b"], g["c"])
        for kw in ({}, {"max_iter": 2}):
            assert cx.solve_raw(_opts(**kw))[0] == (ITERATION_LIMIT if kw else OK)
            rc, y, col, info = _raw_get(cx, 0, m, n)
            assert rc == OK and info.kind == NONE and info.status == (ITERATION_LIMIT if kw else OK)
            assert (y == SENTINEL).all() and (col == SENTINEL).all() and np.isnan(info.scale) and np.isnan(info.residual)
            assert (info.tau, info.kappa) == (cx.duals()["tau"], cx.duals()["kappa"])
        # a lockstep batch: update_lockstep_vectors invalidates; the device entry's refusals
        K = 3
        mems = [batch_member("dense", k, role(k, K)) for k in range(K)]
        G, bs, cs = mems[0][0], [q[1] for q in mems], [q[2] for q in mems]
        cx.upload_lockstep_shared(G, bs, cs)
        assert get() == NO_PROBLEM
        assert [r[0] for r in cx.solve_lockstep(_opts())] == [OK, INFEASIBLE, UNBOUNDED]
        assert get(K - 1) == OK and get(K) == BAD_ARGUMENT
        yd = torch.full((K, m), SENTINEL, dtype=torch.float64, device="cuda")
        cd = torch.full((K, n), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        infos = (_capi.CertInfo * K)()
        dev = lambda yp, ldy, cp, ldc, rec=infos: lib.lpipm_get_certificate_device(cx._h, C.c_void_p(yp) if yp else None, ldy,
                                                                                   C.c_void_p(cp) if cp else None, ldc, rec)
        assert dev(yd.data_ptr(), m, cd.data_ptr(), n, None) == BAD_ARGUMENT         # a null info_out: nothing is written
        assert (yd.cpu().numpy() == SENTINEL).all() and (cd.cpu().numpy() == SENTINEL).all()
        assert dev(yd.data_ptr(), m, cd.data_ptr(), n) == OK
        assert [r.kind for r in infos] == [NONE, FARKAS, RAY]
        assert dev(yd.data_ptr(), m - 1, cd.data_ptr(), n) == BAD_ARGUMENT           # ldy too small
        assert dev(yd.data_ptr(), m, cd.data_ptr(), n - 1) == BAD_ARGUMENT           # ldc too small
        # rows that would end outside the allocation (far outside: torch's allocator hands out parts of larger blocks)
        assert dev(yd.data_ptr(), 1 << 40, cd.data_ptr(), n) == BAD_ARGUMENT
        yh, ch = yd.cpu().numpy(), cd.cpu().numpy()
        assert (yh[0] == SENTINEL).all() and (ch[0] == SENTINEL).all()               # the member with a solution
        assert (yh[1] != SENTINEL).all() and (ch[1] != SENTINEL).all()               # Farkas: y and z
        assert (yh[2] == SENTINEL).all() and (ch[2] != SENTINEL).all()               # ray: x alone
        host = np.zeros((K, m))
        assert dev(host.ctypes.data, m, cd.data_ptr(), n) == BAD_ARGUMENT            # a host pointer
        assert dev(None, 0, None, 0) == OK                                           # nothing asked for: the infos alone
        cx.update_lockstep_vectors(bs, cs)
        assert get() == NO_PROBLEM and dev(yd.data_ptr(), m, cd.data_ptr(), n) == NO_PROBLEM
        assert len(cx.solve_lockstep(_opts())) == K and get(1) == OK
        # a solve that returns a runtime code leaves no certificate either (the QR arms are single-LP: LPIPM_ERR_UNSUPPORTED)
        with pytest.raises(lp_amd.BackendError):
            cx.solve_lockstep(_opts(solver_type=1))
        assert get() == NO_PROBLEM
        # lpipm_solve_batch* leave nothing to ask about
        cx.upload_arrays(A, b, c)
        assert cx.solve_raw(_opts())[0] == INFEASIBLE and get() == OK
        res = cx.solve_batch([(A, b, c, 0.0), (g["A"], g["b"], g["c"], 0.0)], _opts())
        assert [r[0] for r in res] == [INFEASIBLE, OK]
        rc, y, col, info = _raw_get(cx, 0, 4096, 4096)
        assert rc == NO_PROBLEM and (y == SENTINEL).all() and (col == SENTINEL).all() and info.kind == -7
        assert lib.lpipm_get_certificate_device(cx._h, None, 0, None, 0, infos) == NO_PROBLEM
        for call in (cx.certificate, cx.certificates_lockstep, lambda: cx.certificates_device(None, 0, None, 0)):
            with pytest.raises(lp_amd.BackendError):
                call()
        # a column-split context
        cx.upload_column_block(A, b, c, n)
        assert get() == UNSUPPORTED and lib.lpipm_get_certificate_device(cx._h, None, 0, None, 0, infos) == UNSUPPORTED
    finally:
        cx.close()


# ---- 7. the Python drivers ----------------------------------------------------------------------------------------------------------
def test_python_drivers(ctx):
    import lp_amd
    import torch
    from lp_amd import batch
    solver = lp_amd.InteriorPoint.default()
    for which, err_type in (("infeasible", lp_amd.Infeasible), ("unbounded", lp_amd.Unbounded)):
        X, b, Ae, be, c = case_lp(("slack", (24, 32, 8), which))["parts"]
        prob = _problem(X, b, Ae, be, c)
        with pytest.raises(err_type) as plain:
            solver.solve(prob)
        assert not hasattr(plain.value, "certificate")
        with pytest.raises(err_type) as e:
            solver.solve_with_certificate(prob)
        cert = e.value.certificate
        if which == "infeasible":
            assert cert["kind"] == FARKAS and cert["x"] is None
            assert cert["y_ub"].shape == (24,) and cert["y_eq"].shape == (8,) and cert["z"].shape == (32,)
            assert (cert["y_ub"] <= X_TOL).all() and (cert["z"] >= 0).all()      # (a `ub` multiplier is <= 0 up to the residual)
            assert np.abs(X.T @ cert["y_ub"] + Ae.T @ cert["y_eq"] + cert["z"]).max() <= X_TOL
            assert abs(b @ cert["y_ub"] + be @ cert["y_eq"] - 1.0) <= X_TOL
        else:
            assert cert["kind"] == RAY and cert["y_ub"] is None and cert["y_eq"] is None and cert["z"] is None
            assert cert["x"].shape == (32,) and (cert["x"] >= 0).all()
            assert (X @ cert["x"]).max() <= X_TOL and np.abs(Ae @ cert["x"]).max() <= X_TOL and abs(c @ cert["x"] + 1.0) <= X_TOL
        assert cert["residual"] <= X_TOL and cert["scale"] > 0
    # a feasible problem: the plain result
    good = _problem(*case_lp(("slack", (24, 32, 8), "good"))["parts"])
    assert solver.solve_with_certificate(good).x().tobytes() == solver.solve(good).x().tobytes()
    # the batch drivers: 7 members in groups of 3, an infeasible member at position 1 and an unbounded one last
    K = 7
    mems = [batch_member("slack", k, role(k, K)) for k in range(K)]
    X, Ae = mems[0][0], mems[0][2]
    bs, cs = [np.concatenate([q[1], q[3]]) for q in mems], [q[4] for q in mems]
    keys = {"status", "x_slack", "fun", "iterations"}
    plain = batch.solve_shared_ub_eq(X, Ae, bs, cs, ctx=ctx, max_group=3)
    a = batch.solve_shared_ub_eq(X, Ae, bs, cs, ctx=ctx, max_group=3, certificates=True)
    A = slack_form(*mems[0])[0]
    sb, sc = [slack_form(*q)[1] for q in mems], [slack_form(*q)[2] for q in mems]
    s = batch.sweep_shared_matrix(A, sb, sc, ctx=ctx, max_group=3, n_slack=X.shape[0], certificates=True)
    assert [q["status"] for q in a] == [q["status"] for q in s] == [role_status(k, K) for k in range(K)]
    for k, (p, q, r) in enumerate(zip(a, s, plain)):
        assert set(r) == keys and p["status"] == r["status"] and p["iterations"] == r["iterations"]
        if _has_x(p["status"]):
            assert set(p) == set(q) == keys and p["x_slack"].tobytes() == r["x_slack"].tobytes()
            continue
        assert set(p) == set(q) == keys | {"cert_kind", "cert_y", "cert_col", "cert_scale", "cert_residual"}
        assert p["cert_kind"] == q["cert_kind"] == (FARKAS if p["status"] == INFEASIBLE else RAY)
        for got, form in ((p, "shared_ub_eq"), (q, "shared_slack")):
            want = _single_result(ctx, form, k, role(k, K))[3]
            as_cert = dict(kind=got["cert_kind"], status=got["status"], y=got["cert_y"], col=got["cert_col"], scale=got["cert_scale"],
                           residual=got["cert_residual"], tau=0.0, kappa=0.0)
            assert _bits(as_cert)[:6] == want[:6], k
    # solve_device
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64, device="cuda")
    out = batch.solve_device(t(A), t(np.stack(sb)), t(np.stack(sc)), n_slack=X.shape[0], ctx=ctx, max_group=3, certificates=True)
    assert len(out) == 7 and len(batch.solve_device(t(A), t(np.stack(sb)), t(np.stack(sc)), n_slack=X.shape[0], ctx=ctx, max_group=3)) == 4
    st, cy, cc, kinds = out[1], out[4].cpu().numpy(), out[5].cpu().numpy(), out[6]
    assert list(st) == [role_status(k, K) for k in range(K)]
    assert list(kinds) == [{INFEASIBLE: FARKAS, UNBOUNDED: RAY}.get(int(v), NONE) for v in st]
    for k in range(K):
        if kinds[k] == NONE:
            assert np.isnan(cy[k]).all() and np.isnan(cc[k]).all()
        else:
            assert cc[k].tobytes() == s[k]["cert_col"].tobytes()
            assert cy[k].tobytes() == s[k]["cert_y"].tobytes() if kinds[k] == FARKAS else np.isnan(cy[k]).all()


def role_status(k, K):
    return {"infeasible": INFEASIBLE, "unbounded": UNBOUNDED, "good": OK}[role(k, K)]
