"""Lockstep batches that share ONE constraint matrix (lpipm_upload_lockstep_shared): A resident once, every pass over it
serving the whole batch.  Each member must come out exactly as if it had been solved alone -- and bit for bit as the same
batch uploaded with one copy of A per member -- including members that stop at different iterations, the two half-batch
views of a batch of 16 or more, and a context that switches between shared, per-member and single uploads."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _solve_single(A, b, c, c0, o):
    import lp_amd
    single = lp_amd.Context(0)
    single.upload_arrays(A, b, c, c0)
    rc, x, fun, it, _ = single.solve_raw(o)
    single.close()
    return rc, x, fun, it


def _same(r1, r2):
    """two lists of (status, x | None, fun, iterations) agree bit for bit"""
    assert len(r1) == len(r2)
    for i, (a, b) in enumerate(zip(r1, r2)):
        assert a[0] == b[0] and a[3] == b[3], (i, a[0], b[0], a[3], b[3])
        assert (a[1] is None) == (b[1] is None), i
        if a[1] is not None:
            assert np.array_equal(a[1], b[1]), (i, np.abs(a[1] - b[1]).max())
            assert a[2] == b[2] or (np.isnan(a[2]) and np.isnan(b[2])), i


@pytest.mark.parametrize("m,n,count", [(96, 200, 5), (256, 512, 8), (130, 333, 3), (64, 150, 18)])
def test_shared_matches_oracle_single_and_copies(ctx, m, n, count):
    import lp_amd
    from lp_amd import synth
    from oracle import capi as oracle
    A, bs, cs, _ = synth.planted_scenarios(count, m, n, count)
    o = lp_amd.InteriorPoint.default().opts()
    ctx.upload_lockstep_shared(A, bs, cs)
    res = ctx.solve_lockstep(o)
    res2 = ctx.solve_lockstep(o)                                   # resident batch solved again: deterministic
    _same(res, res2)
    for i in range(count):
        ref = oracle.solve(A, bs[i], cs[i])
        st, x, fun, it = res[i]
        assert st == ref["status"] == 0 and it == ref["iterations"], (i, st, it, ref["status"], ref["iterations"])
        assert np.abs(x - ref["x_slack"]).max() <= 1e-6
        rc1, x1, f1, it1 = _solve_single(A, bs[i], cs[i], 0.0, o)
        assert rc1 == 0 and it1 == it and np.array_equal(x1, x), (i, it1, it)
    copies = lp_amd.Context(0)
    copies.upload_lockstep([A] * count, bs, cs)
    _same(res, copies.solve_lockstep(o))
    copies.close()


# A = [[1, -1, 0, 0], [0, 0, 1, 1]]: x1 - x2 = b1, x3 + x4 = b2
_A4 = np.array([[1.0, -1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]])
_MEMBERS = [                                                    # (b, c, c0)
    ((0.0, 1.0), (1.0, 1.0, 1.0, 2.0), 0.0),                      # optimal, unique optimum x = (0, 0, 1, 0)
    ((0.0, 1.0), (-1.0, 0.0, 0.0, 0.0), 0.0),                     # unbounded (x1 = x2 -> inf)
    ((1.0, -1.0), (1.0, 1.0, 1.0, 1.0), 0.0),                     # infeasible (x3 + x4 = -1)
    ((2.0, 3.0), (1.0, 2.0, 3.0, 1.0), 4.5),                      # optimal with c0 != 0
    ((0.5, 100.0), (1.0, 1e-3, 1e3, 1.0), 0.0),                   # needs more iterations than the limit below
]


def test_shared_members_stop_at_different_iterations(ctx):
    import lp_amd
    from lp_amd import _capi
    from oracle import capi as oracle
    bs = [np.array(b) for b, _, _ in _MEMBERS]
    cs = [np.array(c) for _, c, _ in _MEMBERS]
    c0s = [c0 for _, _, c0 in _MEMBERS]
    o = lp_amd.InteriorPoint.custom().max_iter(5).build().opts()
    ctx.upload_lockstep_shared(_A4, bs, cs, c0s)
    res = ctx.solve_lockstep(o)
    its = []
    for i in range(len(_MEMBERS)):
        ref = oracle.solve(_A4, bs[i], cs[i], c0s[i], oracle.default_opts(max_iter=5))
        st, x, fun, it = res[i]
        assert st == ref["status"] and it == ref["iterations"], (i, st, it, ref["status"], ref["iterations"])
        its.append(it)
        if st in (_capi.OK, _capi.ITERATION_LIMIT):
            assert np.abs(x - ref["x_slack"]).max() <= 1e-6
        else:
            assert x is None
    assert [r[0] for r in res] == [_capi.OK, _capi.UNBOUNDED, _capi.INFEASIBLE, _capi.OK, _capi.ITERATION_LIMIT]
    assert np.abs(res[0][1] - np.array([0.0, 0.0, 1.0, 0.0])).max() <= 1e-6
    assert abs(res[3][2] - oracle.solve(_A4, bs[3], cs[3], c0s[3])["fun"]) <= 1e-6
    assert len(set(its)) > 1                                       # the point of the test
    copies = lp_amd.Context(0)
    copies.upload_lockstep([_A4] * len(_MEMBERS), bs, cs, c0s)
    _same(res, copies.solve_lockstep(o))
    copies.close()


def test_shared_c4_shape(built):
    """BASELINE config 4's member shape: 32 x 1024x2048 scenarios on one planted A, shared vs one copy per member."""
    import lp_amd
    from lp_amd import synth
    m, n, K = 1024, 2048, 32
    A, bs, cs, xstars = synth.planted_scenarios(0, m, n, K)
    o = lp_amd.InteriorPoint.default().opts()
    shared, copies = lp_amd.Context(0), lp_amd.Context(0)
    shared.upload_lockstep_shared(A, bs, cs)
    copies.upload_lockstep([A] * K, bs, cs)
    npa = -(-n // 16) * 16
    assert copies.resident_bytes() - shared.resident_bytes() >= 31 * 1024 * npa * 8
    rs, rc = shared.solve_lockstep(o), copies.solve_lockstep(o)
    _same(rs, rc)
    for i, (st, x, fun, it) in enumerate(rs):
        assert st == 0, i
        assert np.abs(A @ x - bs[i]).max() <= 1e-6 * max(1.0, np.abs(bs[i]).max()), i
        assert x.min() >= -1e-12, i
        assert np.abs(x - xstars[i]).max() <= 1e-6, (i, np.abs(x - xstars[i]).max())
    shared.close()
    copies.close()


def test_shared_device_output(ctx):
    import torch
    import lp_amd
    from lp_amd import _capi
    bs = [np.array(b) for b, _, _ in _MEMBERS[:4]]
    cs = [np.array(c) for _, c, _ in _MEMBERS[:4]]
    c0s = [c0 for _, _, c0 in _MEMBERS[:4]]
    o = lp_amd.InteriorPoint.default().opts()
    ctx.upload_lockstep_shared(_A4, bs, cs, c0s)
    host = ctx.solve_lockstep(o)
    stride = 7
    out = torch.full((len(bs), stride), -123.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = ctx.solve_lockstep_device(o, out.data_ptr(), stride)
    torch.cuda.synchronize()
    rows = out.cpu().numpy()
    for i, (st, fun, it) in enumerate(dev):
        assert st == host[i][0] and it == host[i][3], i
        if st == _capi.OK:
            assert np.array_equal(rows[i, :4], host[i][1]) and fun == host[i][2], i
            assert np.all(rows[i, 4:] == -123.0), i
        else:
            assert np.all(rows[i] == -123.0), i                        # no solution: the row is left untouched
    assert dev[2][0] == _capi.INFEASIBLE


def test_shared_context_reuse(built):
    """copies -> shared -> single -> shared (other count) -> shared (same padded shape, smaller m and n) on ONE context:
    every result bit-identical to a fresh context's."""
    import lp_amd
    from lp_amd import synth
    o = lp_amd.InteriorPoint.default().opts()
    A, bs, cs, _ = synth.planted_scenarios(3, 96, 200, 6)
    A2, bs2, cs2, _ = synth.planted_scenarios(4, 90, 197, 4)    # same mp / np as A: the arena is kept, A overwritten

    def run(c, step):
        kind, args = step
        if kind == "copies":
            c.upload_lockstep([args[0]] * len(args[1]), args[1], args[2])
            return c.solve_lockstep(o)
        if kind == "shared":
            c.upload_lockstep_shared(*args)
            return c.solve_lockstep(o)
        c.upload_arrays(*args)
        rc, x, fun, it, _ = c.solve_raw(o)
        return [(rc, x, fun, it)]

    steps = [("copies", (A, bs, cs)), ("shared", (A, bs, cs)), ("single", (A, bs[1], cs[1])),
             ("shared", (A, bs[:3], cs[:3])), ("shared", (A2, bs2[:3], cs2[:3])), ("copies", (A2, bs2, cs2))]
    reused = lp_amd.Context(0)
    for step in steps:
        got = run(reused, step)
        fresh = lp_amd.Context(0)
        want = run(fresh, step)
        fresh.close()
        assert all(r[0] == 0 for r in want), step[0]
        _same(got, want)
    reused.close()


def _ub_members(seed, m_ub, nx, count, m_eq=0):
    """`count` planted LPs min c'x st X x <= b_ub, E x == b_eq, x >= 0 over one X (m_ub x nx) and one E (m_eq x nx): an optimal
    vertex with nx // 2 positive entries and as many active rows.  -> X, E, [b = [b_ub; b_eq]], [c]"""
    rng = np.random.default_rng(seed)
    X, E = rng.standard_normal((m_ub, nx)), rng.standard_normal((m_eq, nx))
    bs, cs = [], []
    for _ in range(count):
        k = nx // 2
        xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
        act = rng.permutation(m_ub)[:k]
        s = rng.uniform(1, 2, m_ub); s[act] = 0.0
        lam = np.zeros(m_ub); lam[act] = rng.uniform(1, 2, k)
        mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
        bs.append(np.concatenate([X @ xs + s, E @ xs]))
        cs.append(-X.T @ lam + mu + E.T @ rng.standard_normal(m_eq))
    return X, E, bs, cs


def test_one_context_through_every_form(built):
    """single dense -> single with hint -> ub_eq -> tall -> lockstep -> lockstep with hint -> shared -> shared with hint -> shared
    ub_eq -> shared tall -> single dense on ONE context, three members to a batch: every step's statuses, iteration counts, fun
    and x bit-identical to the same step on a fresh context."""
    import lp_amd
    from lp_amd import synth
    o = lp_amd.InteriorPoint.default().opts()
    A, bs, cs, _ = synth.planted_scenarios(7, 96, 200, 3)
    X, _, hb, hc = _ub_members(8, 60, 40, 3)                              # the hint: [X I], n_slack = m
    H, hc = np.hstack([X, np.eye(60)]), [np.concatenate([c, np.zeros(60)]) for c in hc]
    Xu, Eu, ub, uc = _ub_members(9, 60, 40, 3, m_eq=30)
    Xt, _, tb, tc = _ub_members(10, 300, 20, 3)
    prob_ue = lp_amd.Problem.target(uc[1]).ub(Xu, ub[1][:60]).eq(Eu, ub[1][60:]).build()
    prob_t = lp_amd.Problem.target(tc[1]).ub(Xt, tb[1]).build()

    def single(c, upload):
        upload(c)
        rc, x, fun, it, _ = c.solve_raw(o)
        return [(rc, x, fun, it)]

    def batch(c, upload):
        upload(c)
        return c.solve_lockstep(o)

    steps = [
        ("single", single, lambda c: c.upload_arrays(A, bs[0], cs[0])),
        ("single hint", single, lambda c: c.upload_arrays(H, hb[0], hc[0], n_slack=60)),
        ("ub_eq", single, lambda c: c.upload(prob_ue)),
        ("tall", single, lambda c: c.upload(prob_t, tall=True)),
        ("lockstep", batch, lambda c: c.upload_lockstep([A] * 3, bs, cs)),
        ("lockstep hint", batch, lambda c: c.upload_lockstep([H] * 3, hb, hc, n_slack=60)),
        ("shared", batch, lambda c: c.upload_lockstep_shared(A, bs, cs)),
        ("shared hint", batch, lambda c: c.upload_lockstep_shared(H, hb, hc, n_slack=60)),
        ("shared ub_eq", batch, lambda c: c.upload_lockstep_shared_ub_eq(Xu, Eu, ub, uc)),
        ("shared tall", batch, lambda c: c.upload_lockstep_shared_ub_tall(Xt, tb, tc)),
        ("single again", single, lambda c: c.upload_arrays(A, bs[2], cs[2])),
    ]
    reused = lp_amd.Context(0)
    for name, run, upload in steps:
        got = run(reused, upload)
        fresh = lp_amd.Context(0)
        want = run(fresh, upload)
        fresh.close()
        assert all(r[0] == 0 for r in want), (name, [r[0] for r in want])
        _same(got, want)
    reused.close()


def test_shared_upload_errors(ctx):
    import lp_amd
    from lp_amd import _capi
    L = _capi.lib()
    m, n, K = 4, 6, 3
    A = np.ones((m, n)); bs = [np.ones(m) for _ in range(K)]; cs = [np.ones(n) for _ in range(K)]
    dp = C.POINTER(C.c_double)
    arr = lambda lst: (dp * len(lst))(*[x.ctypes.data_as(dp) for x in lst])
    pa = A.ctypes.data_as(dp)
    assert L.lpipm_upload_lockstep_shared(ctx._h, K, m, n, None, n, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_upload_lockstep_shared(ctx._h, K, m, n, pa, n, None, arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_upload_lockstep_shared(ctx._h, K, m, n, pa, n, arr(bs), None, None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_upload_lockstep_shared(ctx._h, K, m, n, pa, n - 1, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_upload_lockstep_shared(ctx._h, 0, m, n, pa, n, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_upload_lockstep_shared(ctx._h, K, 0, n, pa, n, arr(bs), arr(cs), None) == _capi.UNCONSTRAINED
    out = C.c_uint64(0)
    assert L.lpipm_get_resident_bytes(None, C.byref(out)) == _capi.ERR_BAD_ARGUMENT
    # the QR arms are single-LP, shared or not
    from lp_amd import synth
    A, bs, cs, _ = synth.planted_scenarios(5, 32, 80, 3)
    ctx.upload_lockstep_shared(A, bs, cs)
    qr = lp_amd.InteriorPoint.custom().solver_type(lp_amd.EquationSolverType.Inverse).build().opts()
    with pytest.raises(lp_amd.BackendError):
        ctx.solve_lockstep(qr)
    assert ctx.resident_bytes() > 0


def test_solve_shared_matrix_groups(built):
    """lp_amd.batch.solve_shared_matrix: 7 members in shared-A groups of at most 3, each as its own single solve."""
    import lp_amd
    from lp_amd import batch, synth
    A, bs, cs, _ = synth.planted_scenarios(6, 80, 170, 7)
    c0s = [0.25 * i for i in range(7)]
    o = lp_amd.InteriorPoint.default().opts()
    ctx = lp_amd.Context(0)
    out = batch.solve_shared_matrix(A, bs, cs, c0s, opts=o, ctx=ctx, max_group=3)
    ctx.close()
    assert len(out) == 7
    for i, r in enumerate(out):
        rc, x, fun, it = _solve_single(A, bs[i], cs[i], c0s[i], o)
        assert r["status"] == rc == 0 and r["iterations"] == it and np.array_equal(r["x_slack"], x) and r["fun"] == fun, i
