"""Lockstep batches of tall LPs with equality rows over ONE image (lpipm_upload_lockstep_shared_ub_eq_tall).

The yardstick is the single tall-eq solve: every member of a batch -- whatever the count, wherever it sits, whichever members
have already stopped, as one view or two half-batch views -- has the status, iteration count, fun and the bytes of x of
Context.upload_tall_eq(problem) + solve_raw of that member alone.  In front of the solves, the one kernel path the batch adds:
the substitution Zt = B.L^-T with a member dimension, through its own entry (k_trsm_lt_lockstep).  Besides: failed pivots, the
oracle, the existing shared path (upload_lockstep_shared_ub_eq), m_eq = 0, new vectors in place, the sweep drivers, device rows,
scaling, memory, the refusals and geometry switches on one context.

Shapes (m_ub, nx, m_eq): (300, 40, 1) and (300, 40, 5) -- nxp 128, one strip of Zt --, (300, 40, 39) -- three 16-row strips with
a ragged last one --, (1100, 130, 17) -- nxp 256: two 128-blocks of L, the update of the rows below runs.  Counts 1, 3 (a short
group), 8 (the XCD-major A.D.A^T grid), 11 (8 + 3) and 19 (two views of 9 and 10, the infeasible member in one, the unbounded
one in the other).  Generator and the conditions on it: tests/test_tall_eq_batch_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_tall_eq_batch_host import (BASE, FAILING, INF, LARGE, LOST, UNB, X_TOL, member_of, oracle_pair, pair_of, specs_of,
                                     vectors_of)

pytestmark = pytest.mark.gpu

dp = C.POINTER(C.c_double)
p = lambda a: a.ctypes.data_as(dp)
arr = lambda lst: (dp * len(lst))(*[p(a) for a in lst])


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _norm(rc, x, fun, it):
    has_x = rc in (0, 7)
    return int(rc), _bits(x) if has_x else None, _bits(np.float64(fun)) if has_x else None, int(it)


def _problem(shape, b, c, X=None, Ae=None):
    import lp_amd
    m = shape[0]
    X0, Ae0 = pair_of(shape)
    return lp_amd.Problem.target(c).ub(X0 if X is None else X, b[:m]).eq(Ae0 if Ae is None else Ae, b[m:]).build()


@functools.lru_cache(maxsize=None)
def _single(shape, spec, kw=()):
    """The single tall-eq solve of one member: computed once per (member, options), shared, immutable."""
    import lp_amd
    b, c = member_of(shape, spec)
    cx = lp_amd.Context(0)
    cx.upload_tall_eq(_problem(shape, b, c))
    rc, x, fun, it, _ = cx.solve_raw(_opts(**dict(kw)))
    cx.close()
    return _norm(rc, x, fun, it)


def _assert_members(res, shape, specs, kw=(), what=""):
    assert len(res) == len(specs)
    for pos, (spec, r) in enumerate(zip(specs, res)):
        got, want = _norm(*r), _single(shape, spec, kw)
        assert got[0] == want[0] and got[3] == want[3], (what, pos, spec, got[0], want[0], got[3], want[3])
        assert got[2] == want[2], (what, pos, spec, "fun")
        assert got[1] == want[1], (what, pos, spec, "x")


def _upload(cx, shape, specs, c0s=None):
    X, Ae = pair_of(shape)
    return cx.upload_lockstep_shared_ub_eq_tall(X, Ae, *vectors_of(shape, specs), c0s)


# ---- 1. the kernel path: Z = B.L^-T with a member dimension ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spd(n, q):
    """Member q's n x n SPD matrix (condition number about 3.5) and numpy's Cholesky factor of it."""
    G = np.random.default_rng(10 * n + q).standard_normal((n, 2 * n))
    M = G @ G.T / (2 * n) + np.eye(n)
    L = np.linalg.cholesky(M)
    M.setflags(write=False); L.setflags(write=False)
    return M, L


@functools.lru_cache(maxsize=None)
def _rhs(n, rows, shared, q):
    """Member q's block of right-hand sides: the one block (n columns) when shared, else its own, three columns short of n."""
    B = np.random.default_rng(1000 * n + 10 * rows + (0 if shared else 1 + q)).standard_normal((rows, n if shared else n - 3))
    B.setflags(write=False)
    return B


def _dot_form(L, B):
    """B.L^-T by forward substitution in dot-product form, column after column of Z: float64 like LAPACK's, its sums in another order."""
    Z = np.zeros((B.shape[0], L.shape[0]))
    Bp = np.zeros_like(Z); Bp[:, :B.shape[1]] = B
    for j in range(L.shape[0]):
        Z[:, j] = (Bp[:, j] - Z[:, :j] @ L[j, :j]) / L[j, j]
    return Z


ROWS = [1, 16, 17, 39]


@functools.lru_cache(maxsize=None)
def _reference(n, rows, shared, q):
    """numpy's B.L^-T (scipy's triangular solve on numpy's factor) and how far the same product summed in another order is from it."""
    import scipy.linalg as sla
    L, B = _spd(n, q)[1], _rhs(n, rows, shared, q)
    Bp = np.zeros((rows, n)); Bp[:, :B.shape[1]] = B
    ref = sla.solve_triangular(L, Bp.T, lower=True, check_finite=False).T
    spread = np.abs(ref - _dot_form(L, B)).max()
    ref.setflags(write=False)
    return ref, spread


def _bound(n, shared, q):
    """4 x the largest such spread over the row counts of the test at this n and matrix: the rounding spread of the product is a
    property of L and of the size of the entries, and the maximum over one row of 128 entries (2.2e-16 = one ulp on some of them)
    does not estimate it; the maximum over the 73 rows of all four cases does."""
    return 4.0 * max(_reference(n, rows, shared, q)[1] for rows in ROWS)


@functools.lru_cache(maxsize=None)
def _alone(n, rows, shared, q):
    """The count-1 call on member q's matrix: a launch without a member dimension, the single kernel."""
    import lp_amd
    Z, info = lp_amd.default_context(0).k_trsm_lt_lockstep(_spd(n, q)[0][None], _rhs(n, rows, shared, q), fill=7.0)
    assert info[0] == 0
    Z.setflags(write=False)
    return Z[0]


def _batch_call(ctx, n, rows, count, shared, mask=None):
    Ms = np.stack([_spd(n, q)[0] for q in range(count)])
    B = _rhs(n, rows, True, 0) if shared else np.stack([_rhs(n, rows, False, q) for q in range(count)])
    Z, infos = ctx.k_trsm_lt_lockstep(Ms, B, done_mask=mask, fill=7.0)
    assert not infos.any()
    return Z


@pytest.mark.parametrize("shared", [True, False], ids=["shared-B", "own-B"])
@pytest.mark.parametrize("count", [1, 3, 8])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", [128, 256, 384])
def test_batched_substitution(ctx, n, rows, count, shared):
    """Every member's Z: the bits of the count-1 call on that member's matrix, and numpy's B.L^-T within the CPU's own spread --
    4 x the largest difference between LAPACK's substitution and the dot-product form of the same product on numpy's factor
    (_bound), which comes to 3.6e-15 .. 7.1e-15 over these matrices (values of Z are O(1); a layout bug gives errors of order 1).
    Rows beyond `rows` and the columns a short B leaves out come back as exact zeros."""
    Z = _batch_call(ctx, n, rows, count, shared)
    rp = -(-rows // 16) * 16
    assert Z.shape == (count, rp, n)
    for q in range(count):
        assert _bits(Z[q]) == _bits(_alone(n, rows, shared, q)), (n, rows, count, shared, q)
        ref, bound = _reference(n, rows, shared, q)[0], _bound(n, shared, q)
        err = np.abs(Z[q, :rows] - ref).max()
        print(f"\n[measure] n {n} rows {rows} count {count} shared {shared} member {q}: max|Z - ref| {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (n, rows, count, shared, q, err, bound)
        assert not Z[q, rows:].any()


@pytest.mark.parametrize("shared", [True, False], ids=["shared-B", "own-B"])
@pytest.mark.parametrize("count", [3, 8])
@pytest.mark.parametrize("n,rows", [(128, 17), (384, 39)])
def test_finished_members_are_not_touched(ctx, n, rows, count, shared):
    """Members 1 and count - 1 marked finished: their Z keep the fill they had before the launch, the others keep their bits."""
    mask = np.zeros(count, dtype=np.int32)
    mask[[1, count - 1]] = 1
    Z = _batch_call(ctx, n, rows, count, shared, mask)
    for q in range(count):
        if mask[q]:
            assert (Z[q] == 7.0).all(), q
        else:
            assert _bits(Z[q]) == _bits(_alone(n, rows, shared, q)), q
    # a batch of one with a mask is the batched kernel on one member: the same bits again, and a finished one is left alone
    one = ctx.k_trsm_lt_lockstep(_spd(n, 0)[0][None], _rhs(n, rows, shared, 0), done_mask=[0], fill=7.0)[0][0]
    assert _bits(one) == _bits(_alone(n, rows, shared, 0))
    assert (ctx.k_trsm_lt_lockstep(_spd(n, 0)[0][None], _rhs(n, rows, shared, 0), done_mask=[1], fill=7.0)[0] == 7.0).all()


# ---- 2. bit-identity to single tall-eq solves ------------------------------------------------------------------------------------
CASES = [(BASE, 1), (BASE, 3), (BASE, 8), (BASE, 11), (BASE, 19), (LARGE, 5), ((300, 40, 1), 3), ((300, 40, 39), 3)]
OPTS = [(), (("ip", 0),), (("max_iter", 3),)]


@pytest.mark.parametrize("kw", OPTS, ids=["default", "ip0", "max_iter3"])
@pytest.mark.parametrize("shape,count", CASES, ids=[f"{s[0]}x{s[1]}+{s[2]}-{k}" for s, k in CASES])
def test_members_are_bit_identical_to_single_tall_eq_solves(ctx, shape, count, kw):
    specs = specs_of(count)
    _upload(ctx, shape, specs)
    assert (ctx.m, ctx.n) == (shape[0] + shape[2], shape[0] + shape[1])
    res = ctx.solve_lockstep(_opts(**dict(kw)))
    _assert_members(res, shape, specs, kw, f"{shape} x {count} {kw}")
    if dict(kw).get("max_iter") == 3:
        assert all(r[3] <= 3 for r in res) and any(r[0] == 7 and not np.isnan(r[1]).any() for r in res)    # IterationLimit, x filled
    else:
        assert sorted({r[0] for r in res}) == ([0, 5, 6] if count >= 3 else [0])
    assert [_norm(*r) for r in res] == [_norm(*r) for r in ctx.solve_lockstep(_opts(**dict(kw)))]      # and again on the same upload


# ---- 3. failed pivots -----------------------------------------------------------------------------------------------------------
def test_more_equality_rows_than_columns(ctx):
    """m_eq = 41 > nx = 40: S is singular by construction; every member is a NumericalProblem in its own pivot word, at the
    iteration the single upload stops at."""
    specs = [0, 1, 2]
    _upload(ctx, FAILING, specs)
    res = ctx.solve_lockstep(_opts())
    for spec, r in zip(specs, res):
        want = _single(FAILING, spec)
        assert want[0] == 2 and (r[0], r[3]) == (want[0], want[3]), (spec, r[0], r[3], want[0], want[3])
    # the context is whole afterwards
    _upload(ctx, BASE, specs_of(3))
    _assert_members(ctx.solve_lockstep(_opts()), BASE, specs_of(3), (), "after the failed pivots")


def test_a_lost_pivot_stays_with_its_member_and_with_its_solve(ctx):
    """A member whose K loses a pivot in its last iteration (a NumericalProblem of the form itself: the host file has the
    condition) in the middle of a batch: its neighbours keep their bits; the same batch solved again gives the same bits again,
    the lost member at the same iteration; and the members that new vectors put in its place are solved as on a fresh upload --
    nothing of the lost solve is left in the member's arena."""
    assert _single(BASE, LOST)[0] == 2                     # (the precondition: the single upload loses it as well)
    specs = [0, LOST, 1, 2, LOST]
    _upload(ctx, BASE, specs)
    first = ctx.solve_lockstep(_opts())
    _assert_members(first, BASE, specs, (), "a lost pivot inside the batch")
    assert [r[0] for r in first] == [0, 2, 0, 0, 2]
    again = ctx.solve_lockstep(_opts())
    assert [_norm(*r) for r in again] == [_norm(*r) for r in first]
    later = [3, 4, 5, LOST, 6]
    ctx.update_lockstep_vectors(*vectors_of(BASE, later))
    _assert_members(ctx.solve_lockstep(_opts()), BASE, later, (), "new members where the pivot was lost")


# ---- 4. against the oracle ------------------------------------------------------------------------------------------------------
def _check_against(pair, got, what):
    """_check_against of tests/test_gpu_tall_eq.py: the oracle's status, an iteration count the oracle produced, x inside the
    oracle's as-generated / permuted envelope widened by X_TOL, fun to 1e-6 relative."""
    ref, alt = pair
    rc, x, fun, it = got
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


def test_batch_of_8_against_the_oracle(ctx):
    specs = specs_of(8)
    _upload(ctx, BASE, specs)
    res = ctx.solve_lockstep(_opts())
    assert [r[0] for r in res] == [0, 5, 0, 0, 0, 0, 0, 6]
    for spec, r in zip(specs, res):
        _check_against(oracle_pair(BASE, spec), r, f"{BASE} member {spec}")


def test_two_large_members_against_the_oracle(ctx):
    specs = specs_of(5)
    _upload(ctx, LARGE, specs)
    res = ctx.solve_lockstep(_opts())
    for pos in (0, 2):                                                         # members 0 and 1
        _check_against(oracle_pair(LARGE, specs[pos]), res[pos], f"{LARGE} member {specs[pos]}")


# ---- 5. against the existing shared path -----------------------------------------------------------------------------------------
def test_agrees_with_upload_lockstep_shared_ub_eq(ctx):
    specs = specs_of(8)
    X, Ae = pair_of(BASE)
    bs, cs = vectors_of(BASE, specs)
    ctx.upload_lockstep_shared_ub_eq(X, Ae, bs, cs)
    old = ctx.solve_lockstep(_opts())
    ctx.upload_lockstep_shared_ub_eq_tall(X, Ae, bs, cs)
    new = ctx.solve_lockstep(_opts())
    assert [r[0] for r in new] == [r[0] for r in old] and [r[3] for r in new] == [r[3] for r in old]
    for o, n in zip(old, new):
        if o[0] == 0:
            err = np.abs(n[1] - o[1]).max()
            print(f"\n[measure] tall-eq batch vs shared ub_eq: max|dx| {err:.3g}")
            assert err <= X_TOL


# ---- 6. m_eq = 0 ----------------------------------------------------------------------------------------------------------------
def test_without_equality_rows_it_is_the_pure_ub_tall_batch(built):
    import lp_amd
    m, nx, _ = BASE
    X = pair_of(BASE)[0]
    bs, cs = vectors_of(BASE, specs_of(8))
    bs = [b[:m] for b in bs]
    out = []
    for up in (lambda cx: cx.upload_lockstep_shared_ub_tall(X, bs, cs),
               lambda cx: cx.upload_lockstep_shared_ub_eq_tall(X, None, bs, cs),
               lambda cx: cx.upload_lockstep_shared_ub_eq_tall(X, np.zeros((0, nx)), bs, cs)):
        cx = lp_amd.Context(0)
        up(cx)
        out.append((cx.resident_bytes(), [_norm(*r) for r in cx.solve_lockstep(_opts())]))
        cx.close()
    assert out[0] == out[1] == out[2]
    assert sorted({r[0] for r in out[0][1]}) == [0, 5, 6]


# ---- 7. new vectors in place, the sweep drivers -----------------------------------------------------------------------------------
def test_update_lockstep_vectors(built):
    import lp_amd
    import torch
    o = _opts()
    X, Ae = pair_of(BASE)
    old, new = specs_of(8), specs_of(8, first=8)          # members 0-7 (with the two other exits), then members 8-15
    (b0, c0), (b1, c1) = vectors_of(BASE, old), vectors_of(BASE, new)
    k1 = [0.25 * i - 1.0 for i in range(8)]
    cx = lp_amd.Context(0)

    def fresh(bs, cs, c0s=None):
        f = lp_amd.Context(0)
        f.upload_lockstep_shared_ub_eq_tall(X, Ae, bs, cs, c0s)
        out = [_norm(*r) for r in f.solve_lockstep(o)]
        f.close()
        return out

    cx.upload_lockstep_shared_ub_eq_tall(X, Ae, b0, c0)
    _assert_members(cx.solve_lockstep(o), BASE, old, (), "first upload")
    cx.update_lockstep_vectors(bs=b1)                                  # b only
    assert [_norm(*r) for r in cx.solve_lockstep(o)] == fresh(b1, c0)
    cx.update_lockstep_vectors(cs=c1)                                  # c only
    res = cx.solve_lockstep(o)
    assert [_norm(*r) for r in res] == fresh(b1, c1)
    _assert_members(res, BASE, new, (), "b then c replaced")
    cx.update_lockstep_vectors(b0, c0)                                 # both
    _assert_members(cx.solve_lockstep(o), BASE, old, (), "both replaced")
    cx.update_lockstep_vectors(b1, c1, k1)                             # and c0
    with_c0 = cx.solve_lockstep(o)
    assert [_norm(*r) for r in with_c0] == fresh(b1, c1, k1)
    assert all(a[0] != 0 or abs((a[2] - r[2]) - k) <= 1e-9 * max(1.0, abs(r[2])) for a, r, k in zip(with_c0, res, k1))
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        cx.update_lockstep_vectors(bs=[np.zeros(BASE[0])] * 8)          # the upload's own form: b of m_ub + m_eq entries
    # the _device variant: packed row blocks on the device, rows longer than the vectors
    m, nx = BASE[0] + BASE[2], BASE[1]
    ldb, ldc = m + 5, nx + 3
    hb, hc = np.full((8, ldb), np.nan), np.full((8, ldc), np.nan)
    hb[:, :m], hc[:, :nx] = np.array(b0), np.array(c0)
    dev = torch.device("cuda", 0)
    tb, tc = torch.from_numpy(hb).to(dev), torch.from_numpy(hc).to(dev)
    torch.cuda.synchronize(dev)
    cx.update_lockstep_vectors_device(tb.data_ptr(), ldb, tc.data_ptr(), ldc, [0.0] * 8)
    _assert_members(cx.solve_lockstep(o), BASE, old, (), "device blocks")
    L = lp_amd._capi.lib()
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert L.lpipm_update_lockstep_vectors_device(cx._h, 8, vp(tb), m - 1, vp(tc), ldc, None) == lp_amd._capi.ERR_BAD_ARGUMENT
    cx.close()


def test_sweep_equals_solve_equals_single(ctx):
    from lp_amd import batch
    specs = specs_of(19)
    X, Ae = pair_of(BASE)
    bs, cs = vectors_of(BASE, specs)
    a = batch.solve_shared_ub_eq_tall(X, Ae, bs, cs, ctx=ctx, max_group=8)
    b = batch.sweep_shared_ub_eq_tall(X, Ae, bs, cs, ctx=ctx, max_group=8)
    tup = lambda rs: [(r["status"], r["x_slack"], r["fun"], r["iterations"]) for r in rs]
    _assert_members(tup(a), BASE, specs, (), "solve_shared_ub_eq_tall")
    _assert_members(tup(b), BASE, specs, (), "sweep_shared_ub_eq_tall")


# ---- 8. solutions left on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [8, 19])
def test_solve_lockstep_device(ctx, count):
    import torch
    _upload(ctx, BASE, specs_of(count))
    host = ctx.solve_lockstep(_opts())
    n, stride = ctx.n, ctx.n + 7
    dev = torch.device("cuda", 0)
    rows = torch.full((count, stride), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    res = ctx.solve_lockstep_device(_opts(), rows.data_ptr(), stride)
    got = rows.cpu().numpy()
    for i, ((rc, x, fun, it), (rcd, fund, itd)) in enumerate(zip(host, res)):
        assert (rc, it) == (rcd, itd) and _bits(fun) == _bits(fund), i
        if x is None:
            assert rc in (5, 6) and np.all(got[i] == -7.0), i             # the sentinel stays
        else:
            assert _bits(got[i, :n]) == _bits(x) and np.all(got[i, n:] == -7.0), i


# ---- 9. scaling -----------------------------------------------------------------------------------------------------------------
def test_scaling(built):
    import lp_amd
    m, nx, me = BASE
    X, Ae = pair_of(BASE)
    rng = np.random.default_rng(7)
    er, ec = rng.integers(-16, 17, m + me), rng.integers(-16, 17, nx)
    Xd, Aed = np.ldexp(X, er[:m, None] + ec[None, :]), np.ldexp(Ae, er[m:, None] + ec[None, :])
    specs = specs_of(8)
    bs, cs = vectors_of(BASE, specs)
    bs, cs = [np.ldexp(b, er) for b in bs], [np.ldexp(c, ec) for c in cs]
    o = _opts()
    cx = lp_amd.Context(0).set_scaling(8)
    cx.upload_lockstep_shared_ub_eq_tall(Xd, Aed, bs, cs)
    kr, kc = cx.scaling(0)
    res = [_norm(*r) for r in cx.solve_lockstep(o)]
    assert np.any(kr[:m] != 0) and np.any(kr[m:] != 0) and np.any(kc[:nx] != 0)
    one = lp_amd.Context(0).set_scaling(8)
    for i in range(8):
        one.upload_tall_eq(_problem(BASE, bs[i], cs[i], Xd, Aed))
        if i == 0:
            kr1, kc1 = one.scaling()
            assert np.array_equal(kr, kr1) and np.array_equal(kc, kc1)       # one set of exponents: the single upload's
        rc, x, fun, it, _ = one.solve_raw(o)
        assert res[i] == _norm(rc, x, fun, it), (i, res[i][0], rc, res[i][3], it)
    assert sorted({r[0] for r in res}) == [0, 5, 6]
    # ... and later vectors are scaled with the kept exponents
    cx.update_lockstep_vectors(bs[::-1], cs[::-1])
    assert [_norm(*r) for r in cx.solve_lockstep(o)] == res[::-1]
    one.close(); cx.close()


# ---- 10. memory -----------------------------------------------------------------------------------------------------------------
def test_resident_bytes(built):
    import lp_amd
    KIB64 = 64 << 10
    m, nx, me = LARGE

    def resident(shape, count):
        cx = lp_amd.Context(0)
        X, Ae = pair_of(shape)
        b, c = np.ones(shape[0] + shape[2]), np.ones(shape[1])
        if count:
            cx.upload_lockstep_shared_ub_eq_tall(X, Ae, [b] * count, [c] * count)
        else:
            cx.upload_tall_eq(_problem(shape, b, c))
        out = cx.resident_bytes()
        cx.close()
        return out

    mp, npa, nxp, mk = 1152, 144, 256, 1104
    single, two, four, eight = resident(LARGE, 0), resident(LARGE, 2), resident(LARGE, 4), resident(LARGE, 8)
    per_member = (eight - four) // 4
    print(f"\n[measure] resident bytes at {LARGE}: single {single}, batches of 2 / 4 / 8: {two} / {four} / {eight}: {per_member} per added member")
    assert (four - two) == 2 * per_member and (eight - four) == 4 * per_member            # equal increments
    assert per_member <= single - 8 * (mp * npa + nxp * mk) + KIB64, (per_member, single)   # no copy of the image or of Xt in a member
    twice = resident((2 * m, nx, me), 8)
    print(f"[measure] resident bytes, count 8: m_ub = {m}: {eight}, m_ub = {2 * m}: {twice}")
    assert twice < 2 * eight + 8 * KIB64, (eight, twice)                                    # nothing grows as m_ub^2


# ---- 11. refusals and geometry switches ------------------------------------------------------------------------------------------
class _NeverCalled:
    """An all-reduce for lpipm_set_collective that no refused upload may reach."""
    def __init__(self):
        from lp_amd import _capi
        self.calls = 0
        self.cfn = _capi.ALLREDUCE_FN(self._call)

    def _call(self, *args):
        self.calls += 1
        return 1


def _raw(cx, count, nx, m, X, lda, me, Ae, lde, bs, cs):
    from lp_amd import _capi
    return _capi.lib().lpipm_upload_lockstep_shared_ub_eq_tall(cx._h, count, nx, m, X, lda, me, Ae, lde, bs, cs, None)


def test_refusals_and_codes(built, monkeypatch):
    import lp_amd
    from lp_amd import _capi
    L = _capi.lib()
    m, nx, me = BASE
    X, Ae = [np.ascontiguousarray(a) for a in pair_of(BASE)]
    specs = specs_of(3)
    bs, cs = [[np.ascontiguousarray(a) for a in v] for v in vectors_of(BASE, specs)]
    B, Cs = arr(bs), arr(cs)
    null_row = (dp * 3)(p(bs[0]), None, p(bs[2]))
    OKC, BAD, UNS, UNC = _capi.OK, _capi.ERR_BAD_ARGUMENT, _capi.ERR_UNSUPPORTED, _capi.UNCONSTRAINED
    refused = [((3, nx, 0, None, nx, 0, None, nx, B, Cs), UNC), ((3, nx, 0, None, nx, me, p(Ae), nx, B, Cs), UNS),
               ((0, nx, m, p(X), nx, me, p(Ae), nx, B, Cs), BAD), ((4097, nx, m, p(X), nx, me, p(Ae), nx, arr(bs * 1366), arr(cs * 1366)), BAD),
               ((3, nx, m, None, nx, me, p(Ae), nx, B, Cs), BAD), ((3, nx, m, p(X), nx, me, None, nx, B, Cs), BAD),
               ((3, nx, m, p(X), nx, me, p(Ae), nx, None, Cs), BAD), ((3, nx, m, p(X), nx, me, p(Ae), nx, B, None), BAD),
               ((3, nx, m, p(X), nx - 1, me, p(Ae), nx, B, Cs), BAD), ((3, nx, m, p(X), nx, me, p(Ae), nx - 1, B, Cs), BAD),
               ((3, nx, m, p(X), nx, me, p(Ae), nx, null_row, Cs), BAD)]
    cx = lp_amd.Context(0)
    for args, code in refused:                                       # on an empty context: nothing becomes resident
        assert _raw(cx, *args) == code, (args[:3], code)
        assert cx.resident_bytes() == 0
    _upload(cx, BASE, specs)
    want = [_norm(*r) for r in cx.solve_lockstep(_opts())]
    _assert_members(cx.solve_lockstep(_opts()), BASE, specs, (), "before the refusals")
    for args, code in refused:                                       # on a resident batch: it solves to the same bits afterwards
        assert _raw(cx, *args) == code, (args[:3], code)
        assert [_norm(*r) for r in cx.solve_lockstep(_opts())] == want, args[:3]
    # the QR arms at solve time, the single-LP kernel entries and the single-LP update on the batch
    for st in (1, 2):
        with pytest.raises(lp_amd.BackendError):
            cx.solve_lockstep(_opts(solver_type=st))
        held = [np.empty(m + nx) for _ in range(3)]
        assert L.lpipm_solve_lockstep(cx._h, C.byref(_opts(solver_type=st)), arr(held), None, None, (C.c_int32 * 3)()) == UNS
    n, mm = m + nx, m + me
    d, K, M, S = np.ones(n), np.empty((nx, nx)), np.empty((mm, mm)), np.empty((me, me))
    x, y, z, tk = np.ones(n), np.ones(mm), np.ones(n), np.ones(2)
    one = C.c_double(1.0)
    for count in (3, 1):                                             # (a batch of ONE is a batch too)
        _upload(cx, BASE, specs[:count])
        assert L.lpipm_k_tall_normal(cx._h, p(d), p(K)) == UNS
        assert L.lpipm_k_tall_schur(cx._h, p(d), p(S)) == UNS
        assert L.lpipm_k_tall_sym_solve(cx._h, p(d), 1, p(np.ones(n)), p(np.ones(mm)), p(np.empty(n)), p(np.empty(mm)), None) == UNS
        assert L.lpipm_k_adat(cx._h, p(d), p(M), 1, None) == UNS
        assert L.lpipm_k_iteration(cx._h, C.byref(_opts()), 0, p(x), p(y), p(z), C.byref(one), C.byref(one), p(np.empty(n)),
                                   p(np.empty(mm)), p(np.empty(n)), p(tk), C.byref(one), None) == UNS
        assert L.lpipm_update_vectors(cx._h, p(np.ones(mm)), p(np.ones(n))) == UNS
    _upload(cx, BASE, specs)
    assert [_norm(*r) for r in cx.solve_lockstep(_opts())] == want
    cx.close()
    # a column-split context and a refining one
    cx = lp_amd.Context(0)
    coll = _NeverCalled()
    cx.set_collective(1, 2, coll)
    assert _raw(cx, 3, nx, m, p(X), nx, me, p(Ae), nx, B, Cs) == UNS
    assert cx.resident_bytes() == 0 and coll.calls == 0
    cx.set_collective(0, 1, None)                                    # the same context without the split takes the batch
    assert _raw(cx, 3, nx, m, p(X), nx, me, p(Ae), nx, B, Cs) == OKC
    cx._lock = (3, mm, n, None, bs, cs)
    assert [_norm(*r) for r in cx.solve_lockstep(_opts())] == want
    cx.close()
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_REFINE", "2")
    cx = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_REFINE")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    assert _raw(cx, 3, nx, m, p(X), nx, me, p(Ae), nx, B, Cs) == UNS
    assert cx.resident_bytes() == 0
    cx.close()


def test_geometry_switches(built):
    """Single tall-eq -> this batch -> a plain dense upload on ONE context: each solves as on a fresh context."""
    import lp_amd
    from lp_amd import synth
    specs = specs_of(3)
    A, b2, c2, _ = synth.planted_lp(3, 64, 160)
    fresh = lp_amd.Context(0)
    fresh.upload_arrays(A, b2, c2)
    dense = _norm(*fresh.solve_raw(_opts())[:4])
    fresh.close()
    b, c = member_of(BASE, 0)
    cx = lp_amd.Context(0)
    for _ in range(2):                                               # ... and round again: the batch after the dense upload
        cx.upload_tall_eq(_problem(BASE, b, c))
        assert _norm(*cx.solve_raw(_opts())[:4]) == _single(BASE, 0)
        _upload(cx, BASE, specs)
        _assert_members(cx.solve_lockstep(_opts()), BASE, specs, (), "batch after the single tall-eq upload")
        cx.upload_arrays(A, b2, c2)
        assert _norm(*cx.solve_raw(_opts())[:4]) == dense
    cx.close()
