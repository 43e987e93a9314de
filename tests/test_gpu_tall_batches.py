"""Lockstep batches of tall inequality-form LPs over ONE matrix (lpipm_upload_lockstep_shared_ub_tall).

The yardstick is the single tall solve: every member of a batch -- whatever the count, wherever it sits, whichever members
have already stopped, as one view or two half-batch views -- has the status, iteration count, fun and the bytes of x of
Context.upload(problem, tall=True) + solve_raw of that member alone.  The batches hold members that stop at different
iterations and through different exits (optimal, infeasible, unbounded, iteration limit).  Besides: the oracle on the slack form,
the existing shared path (upload_lockstep_shared_ub_eq), new vectors in place, the sweep drivers, device rows, scaling, memory,
geometry switches on one context and the refusals.

Shapes: (300, 40) -- mp 384, mk 304, npa 48, nxp 128, 3 row splits, no multiple of any tile -- and (1100, 130) -- mp 1152 (the
m > 1024 variants of the shared passes), nxp 256 (two diagonal blocks of K), npa 144.  Counts 1, 3 (a short group), 8 (the
XCD-major A.D.A^T grid), 11 (8 + 3) and 19 (two views of 9 and 10)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-6                     # the tall form's own bound against the oracle (tests/test_gpu_tall_form.py)
SMALL, LARGE = (300, 40), (1100, 130)
INF, UNB = "infeasible", "unbounded"


# ---- generator --------------------------------------------------------------------------------------------------------------------
def shared_X(seed, m, nx):       # row 0 >= 0 and column 0 <= 0: lets one member be infeasible, one unbounded
    rng = np.random.default_rng(seed); X = rng.standard_normal((m, nx))
    X[0, :] = np.abs(X[0, :]); X[:, 0] = -np.abs(X[:, 0]); X[0, 0] = 0.0
    return X


def member(X, seed):             # planted(...) of tests/test_gpu_tall_form.py on a GIVEN X -> b, c
    rng = np.random.default_rng(seed)
    m, nx = X.shape
    k = nx // 2
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:k]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, k)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    return b, -X.T @ lam + mu


@functools.lru_cache(maxsize=None)
def _X(shape):
    X = shared_X(100 + shape[0], *shape)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _member(shape, spec):
    """spec: an int i -- member i of the shape -- or INF / UNB: member 0 with b[0] = -1 / c[0] = -1.  -> b, c"""
    i = spec if isinstance(spec, int) else 0
    b, c = member(_X(shape), 1000 * shape[0] + i)
    if spec == INF:
        b[0] = -1.0              # row 0 of X is >= 0 and x >= 0
    if spec == UNB:
        c[0] = -1.0              # column 0 of X is <= 0
    b.setflags(write=False); c.setflags(write=False)
    return b, c


def _specs(count, first=0):
    """The members of a batch of `count`: optimal members first, first + 1, ...; from count 3 on the infeasible member at
    position 1 and the unbounded one last (in a batch of 19: one in each half)."""
    specs = list(range(first, first + count))
    if count >= 3:
        specs = [first, INF] + list(range(first + 1, first + count - 2)) + [UNB]
    return specs


def _vectors(shape, specs):
    ms = [_member(shape, s) for s in specs]
    return [m[0] for m in ms], [m[1] for m in ms]


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


@functools.lru_cache(maxsize=None)
def _single(shape, spec, kw=()):
    """The single tall solve of one member: computed once per (member, options), shared, immutable."""
    import lp_amd
    b, c = _member(shape, spec)
    cx = lp_amd.Context(0)
    cx.upload(lp_amd.Problem.target(c).ub(_X(shape), b).build(), tall=True)
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


# ---- 1. bit-identity to single tall solves --------------------------------------------------------------------------------------------
CASES = [(SMALL, 1), (SMALL, 3), (SMALL, 8), (SMALL, 11), (SMALL, 19), (LARGE, 5)]
OPTS = [(), (("ip", 0),), (("max_iter", 3),)]


@pytest.mark.parametrize("kw", OPTS, ids=["default", "ip0", "max_iter3"])
@pytest.mark.parametrize("shape,count", CASES, ids=[f"{s[0]}x{s[1]}-{k}" for s, k in CASES])
def test_members_are_bit_identical_to_single_tall_solves(ctx, shape, count, kw):
    specs = _specs(count)
    ctx.upload_lockstep_shared_ub_tall(_X(shape), *_vectors(shape, specs))
    assert (ctx.m, ctx.n) == (shape[0], shape[0] + shape[1])
    res = ctx.solve_lockstep(_opts(**dict(kw)))
    _assert_members(res, shape, specs, kw, f"{shape} x {count} {kw}")
    if dict(kw).get("max_iter") == 3:
        for spec, r in zip(specs, res):
            if isinstance(spec, int):
                assert r[0] == 7 and r[3] == 3 and not np.isnan(r[1]).any()          # IterationLimit, x filled
    else:
        assert sorted({r[0] for r in res}) == ([0, 5, 6] if count >= 3 else [0])
    assert _norm(*res[0]) == _norm(*ctx.solve_lockstep(_opts(**dict(kw)))[0])         # and again on the same upload


@pytest.mark.parametrize("count", [2, 8, 17], ids=["2", "8-xcd-major", "17-two-views"])
def test_a_plan_that_a_single_lp_runs_on_the_round2_kernel(built, count):
    """nxp = 768 (21 tiles of K) and 257 k-tiles: the single LP's K comes from the round-2 kernel with a contraction longer than
    the canonical chunking covers, whose bits depend on its workgroup count -- the batch runs that very plan, also on the
    XCD-major grid (count 8) and under half-batch views (count 17: views of 8 and 9, bt.first > 0).  Members repeat: only two
    single solves are needed."""
    import lp_amd
    shape = (4100, 650)
    specs = [i % 2 for i in range(count)]
    cx = lp_amd.Context(0)
    cx.upload_lockstep_shared_ub_tall(_X(shape), *_vectors(shape, specs))
    res = cx.solve_lockstep(_opts(max_iter=4))
    cx.close()
    _assert_members(res, shape, specs, (("max_iter", 4),), "round-2 plan")


# ---- 2. against the oracle ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(shape, spec):
    from oracle import capi as oracle
    X = _X(shape)
    b, c = _member(shape, spec)
    m, nx = shape
    ref = oracle.solve(np.hstack([X, np.eye(m)]), b, np.concatenate([c, np.zeros(m)]), want_log=False)
    if ref["x_slack"] is not None:
        ref["x_slack"].setflags(write=False)
    return ref


def _check_oracle(shape, specs, res):
    for spec, (rc, x, fun, it) in zip(specs, res):
        ref = _oracle(shape, spec)
        print(f"\n[measure] {shape} member {spec}: status {rc} / oracle {ref['status']}, iterations {it} / oracle {ref['iterations']}")
        assert rc == ref["status"], (spec, rc, ref["status"])
        if rc != 0:
            continue             # (their iteration counts are held to the single tall solve by test 1)
        err, frel = np.abs(x - ref["x_slack"]).max(), abs(fun - ref["fun"]) / max(1.0, abs(ref["fun"]))
        print(f"[measure]   max|x - x_oracle| {err:.3g}, fun rel {frel:.3g}")
        assert it == ref["iterations"], (spec, it, ref["iterations"])
        assert err <= X_TOL and frel <= 1e-6, (spec, err, frel)


def test_batch_of_8_against_the_oracle(ctx):
    specs = _specs(8)
    ctx.upload_lockstep_shared_ub_tall(_X(SMALL), *_vectors(SMALL, specs))
    res = ctx.solve_lockstep(_opts())
    assert [r[0] for r in res] == [0, 5, 0, 0, 0, 0, 0, 6]
    _check_oracle(SMALL, specs, res)


def test_two_large_members_against_the_oracle(ctx):
    specs = _specs(5)
    ctx.upload_lockstep_shared_ub_tall(_X(LARGE), *_vectors(LARGE, specs))
    res = ctx.solve_lockstep(_opts())
    _check_oracle(LARGE, [specs[0], specs[2]], [res[0], res[2]])              # members 0 and 1


# ---- 3. against the existing shared path ---------------------------------------------------------------------------------------------
def test_agrees_with_upload_lockstep_shared_ub_eq(ctx):
    specs = _specs(8)
    bs, cs = _vectors(SMALL, specs)
    ctx.upload_lockstep_shared_ub_eq(_X(SMALL), None, bs, cs)
    old = ctx.solve_lockstep(_opts())
    ctx.upload_lockstep_shared_ub_tall(_X(SMALL), bs, cs)
    new = ctx.solve_lockstep(_opts())
    assert [r[0] for r in new] == [r[0] for r in old] and [r[3] for r in new] == [r[3] for r in old]
    for o, n in zip(old, new):
        if o[0] == 0:
            err = np.abs(n[1] - o[1]).max()
            print(f"\n[measure] tall batch vs shared ub_eq: max|dx| {err:.3g}")
            assert err <= X_TOL


# ---- 4. new vectors in place ---------------------------------------------------------------------------------------------------------
def test_update_lockstep_vectors(built):
    import lp_amd
    import torch
    o = _opts()
    old, new = _specs(8), _specs(8, first=8)          # members 0-7 (with the two other exits), then members 8-15
    (b0, c0), (b1, c1) = _vectors(SMALL, old), _vectors(SMALL, new)
    k1 = [0.25 * i - 1.0 for i in range(8)]
    cx = lp_amd.Context(0)

    def fresh(bs, cs, c0s=None):
        f = lp_amd.Context(0)
        f.upload_lockstep_shared_ub_tall(_X(SMALL), bs, cs, c0s)
        out = [_norm(*r) for r in f.solve_lockstep(o)]
        f.close()
        return out

    cx.upload_lockstep_shared_ub_tall(_X(SMALL), b0, c0)
    _assert_members(cx.solve_lockstep(o), SMALL, old, (), "first upload")
    cx.update_lockstep_vectors(bs=b1)
    assert [_norm(*r) for r in cx.solve_lockstep(o)] == fresh(b1, c0)
    cx.update_lockstep_vectors(cs=c1)
    res = cx.solve_lockstep(o)
    assert [_norm(*r) for r in res] == fresh(b1, c1)
    _assert_members(res, SMALL, new, (), "b then c replaced")
    cx.update_lockstep_vectors(b0, c0)
    cx.update_lockstep_vectors(b1, c1, k1)
    with_c0 = cx.solve_lockstep(o)
    assert [_norm(*r) for r in with_c0] == fresh(b1, c1, k1)
    assert all(a[0] != 0 or abs((a[2] - r[2]) - k) <= 1e-9 * max(1.0, abs(r[2])) for a, r, k in zip(with_c0, res, k1))
    k0 = [0.0] * 8
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        cx.update_lockstep_vectors(cs=[np.zeros(SMALL[0] + SMALL[1])] * 8)        # the lockstep form: the n structural costs
    # the _device variant: packed row blocks on the device, rows longer than the vectors
    m, nx = SMALL
    ldb, ldc = m + 5, nx + 3
    hb, hc = np.full((8, ldb), np.nan), np.full((8, ldc), np.nan)
    hb[:, :m], hc[:, :nx] = np.array(b0), np.array(c0)
    dev = torch.device("cuda", 0)
    tb, tc = torch.from_numpy(hb).to(dev), torch.from_numpy(hc).to(dev)
    torch.cuda.synchronize(dev)
    cx.update_lockstep_vectors_device(tb.data_ptr(), ldb, tc.data_ptr(), ldc, k0)
    _assert_members(cx.solve_lockstep(o), SMALL, old, (), "device blocks")
    L = lp_amd._capi.lib()
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert L.lpipm_update_lockstep_vectors_device(cx._h, 8, vp(tb), ldb, vp(tc), nx - 1, None) == lp_amd._capi.ERR_BAD_ARGUMENT
    cx.close()


# ---- 5. the sweep drivers --------------------------------------------------------------------------------------------------------------
def test_sweep_equals_solve_equals_single(ctx):
    from lp_amd import batch
    specs = _specs(11)
    bs, cs = _vectors(SMALL, specs)
    a = batch.solve_shared_ub_tall(_X(SMALL), bs, cs, ctx=ctx, max_group=4)
    b = batch.sweep_shared_ub_tall(_X(SMALL), bs, cs, ctx=ctx, max_group=4)
    tup = lambda rs: [(r["status"], r["x_slack"], r["fun"], r["iterations"]) for r in rs]
    _assert_members(tup(a), SMALL, specs, (), "solve_shared_ub_tall")
    _assert_members(tup(b), SMALL, specs, (), "sweep_shared_ub_tall")


# ---- 6. solutions left on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [8, 19])
def test_solve_lockstep_device(ctx, count):
    import torch
    specs = _specs(count)
    ctx.upload_lockstep_shared_ub_tall(_X(SMALL), *_vectors(SMALL, specs))
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


# ---- 7. scaling ----------------------------------------------------------------------------------------------------------------------
def test_scaling(built):
    import lp_amd
    m, nx = SMALL
    rng = np.random.default_rng(7)
    er, ec = rng.integers(-12, 13, m), rng.integers(-12, 13, nx)
    Xd = np.ldexp(_X(SMALL), er[:, None] + ec[None, :])
    specs = _specs(8)
    bs, cs = _vectors(SMALL, specs)
    bs, cs = [np.ldexp(b, er) for b in bs], [np.ldexp(c, ec) for c in cs]
    o = _opts()
    cx = lp_amd.Context(0).set_scaling(8)
    cx.upload_lockstep_shared_ub_tall(Xd, bs, cs)
    kr, kc = cx.scaling(0)
    res = [_norm(*r) for r in cx.solve_lockstep(o)]
    assert np.any(kr != 0) and np.any(kc[:nx] != 0)
    one = lp_amd.Context(0).set_scaling(8)
    for i in range(8):
        one.upload(lp_amd.Problem.target(cs[i]).ub(Xd, bs[i]).build(), tall=True)
        if i == 0:
            kr1, kc1 = one.scaling()
            assert np.array_equal(kr, kr1) and np.array_equal(kc, kc1)
        rc, x, fun, it, _ = one.solve_raw(o)
        assert res[i] == _norm(rc, x, fun, it), (i, res[i][0], rc, res[i][3], it)
    # ... and later vectors are scaled with the kept exponents
    cx.update_lockstep_vectors(bs[::-1], cs[::-1])
    assert [_norm(*r) for r in cx.solve_lockstep(o)] == res[::-1]
    one.close(); cx.close()


# ---- 8. memory -----------------------------------------------------------------------------------------------------------------------
def test_resident_bytes(built):
    import lp_amd
    KIB64 = 64 << 10

    def resident(shape, count):
        cx = lp_amd.Context(0)
        X = _X(shape)
        bs, cs = [np.ones(shape[0])] * count, [np.ones(shape[1])] * count
        if count:
            cx.upload_lockstep_shared_ub_tall(X, bs, cs)
        else:
            cx.upload(lp_amd.Problem.target(np.ones(shape[1])).ub(X, np.ones(shape[0])).build(), tall=True)
        out = cx.resident_bytes()
        cx.close()
        return out

    m, nx = LARGE
    mp, npa, nxp, mk = 1152, 144, 256, 1104
    single, one, eight = resident(LARGE, 0), resident(LARGE, 1), resident(LARGE, 8)
    per_member = (eight - one) / 7
    print(f"\n[measure] resident bytes at {LARGE}: single {single}, batch of 1 {one}, of 8 {eight}: {per_member:.0f} per added member")
    assert per_member <= single - 8 * (mp * npa + nxp * mk) + KIB64, (per_member, single)      # no copy of X or Xt in a member
    twice = resident((2 * m, nx), 8)
    print(f"[measure] resident bytes, count 8: m = {m}: {eight}, m = {2 * m}: {twice}")
    assert twice < 2 * eight + 8 * KIB64, (eight, twice)                                        # nothing grows as m^2


# ---- 9. geometry switches on one context ------------------------------------------------------------------------------------------------
def _other_uploads():
    import lp_amd
    from lp_amd import synth
    b, c = _member(SMALL, 0)
    A, b2, c2, _ = synth.planted_lp(3, 64, 160)
    bs, cs = _vectors(SMALL, _specs(3))
    return [("single tall", lambda cx: cx.upload(lp_amd.Problem.target(c).ub(_X(SMALL), b).build(), tall=True),
             lambda cx: [_norm(*cx.solve_raw(_opts())[:4])]),
            ("dense", lambda cx: cx.upload_arrays(A, b2, c2), lambda cx: [_norm(*cx.solve_raw(_opts())[:4])]),
            ("shared ub_eq", lambda cx: cx.upload_lockstep_shared_ub_eq(_X(SMALL), None, bs, cs),
             lambda cx: [_norm(*r) for r in cx.solve_lockstep(_opts())])]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["single-tall", "dense", "shared-ub-eq"])
def test_geometry_switches(built, which):
    import lp_amd
    name, upload, solve = _other_uploads()[which]
    specs = _specs(3)
    fresh = lp_amd.Context(0)
    upload(fresh)
    want = solve(fresh)
    fresh.close()
    cx = lp_amd.Context(0)
    cx.upload_lockstep_shared_ub_tall(_X(SMALL), *_vectors(SMALL, specs))
    _assert_members(cx.solve_lockstep(_opts()), SMALL, specs, (), "tall batch first")
    upload(cx)
    assert solve(cx) == want, name                                  # the other upload after a tall batch ...
    cx.upload_lockstep_shared_ub_tall(_X(SMALL), *_vectors(SMALL, specs))
    _assert_members(cx.solve_lockstep(_opts()), SMALL, specs, (), f"tall batch after {name}")     # ... and the reverse order
    cx.close()


# ---- 10. refusals and codes -----------------------------------------------------------------------------------------------------------
def test_refusals_and_codes(built):
    import lp_amd
    from lp_amd import _capi
    L = _capi.lib()
    dp = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    m, nx = SMALL
    X = np.ascontiguousarray(_X(SMALL))
    specs = _specs(3)
    bs, cs = _vectors(SMALL, specs)
    bs, cs = [np.ascontiguousarray(b) for b in bs], [np.ascontiguousarray(c) for c in cs]
    arr = lambda lst: (dp * len(lst))(*[p(a) for a in lst])
    cx = lp_amd.Context(0)
    up = L.lpipm_upload_lockstep_shared_ub_tall
    assert up(cx._h, 3, nx, 0, None, nx, arr(bs), arr(cs), None) == _capi.UNCONSTRAINED
    assert up(cx._h, 0, nx, m, p(X), nx, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, None, nx, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, p(X), nx, None, arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, p(X), nx, arr(bs), None, None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, p(X), nx - 1, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    null_row = (dp * 3)(p(bs[0]), None, p(bs[2]))
    assert up(cx._h, 3, nx, m, p(X), nx, null_row, arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert cx.resident_bytes() == 0
    cx.set_first_factor_cache(False)                                 # a no-op for this batch: no first factor is kept
    cx.upload_lockstep_shared_ub_tall(X, bs, cs)
    off = cx.resident_bytes()
    _assert_members(cx.solve_lockstep(_opts()), SMALL, specs, (), "first-factor cache off")
    cx.set_first_factor_cache(True)
    cx.upload_lockstep_shared_ub_tall(X, bs, cs)
    assert cx.resident_bytes() == off
    for st in (1, 2):
        with pytest.raises(lp_amd.BackendError):
            cx.solve_lockstep(_opts(solver_type=st))
        held = [np.empty(m + nx) for _ in range(3)]
        xs = (dp * 3)(*[p(a) for a in held])
        assert L.lpipm_solve_lockstep(cx._h, C.byref(_opts(solver_type=st)), xs, None, None, (C.c_int32 * 3)()) == _capi.ERR_UNSUPPORTED
    n = m + nx
    d, K, M = np.ones(n), np.empty((nx, nx)), np.empty((m, m))
    assert L.lpipm_k_tall_normal(cx._h, p(d), p(K)) == _capi.ERR_UNSUPPORTED
    U, V = np.empty(n), np.empty(m)
    assert L.lpipm_k_tall_sym_solve(cx._h, p(d), 1, p(np.ones(n)), p(np.ones(m)), p(U), p(V), None) == _capi.ERR_UNSUPPORTED
    assert L.lpipm_k_adat(cx._h, p(d), p(M), 1, None) == _capi.ERR_UNSUPPORTED
    x, y, z, tk = np.ones(n), np.ones(m), np.ones(n), np.ones(2)
    one = C.c_double(1.0)
    assert L.lpipm_k_iteration(cx._h, C.byref(_opts()), 0, p(x), p(y), p(z), C.byref(one), C.byref(one), p(np.empty(n)),
                               p(np.empty(m)), p(np.empty(n)), p(tk), C.byref(one), None) == _capi.ERR_UNSUPPORTED
    # a batch of ONE is a batch too
    cx.upload_lockstep_shared_ub_tall(X, bs[:1], cs[:1])
    assert L.lpipm_k_tall_normal(cx._h, p(d), p(K)) == _capi.ERR_UNSUPPORTED
    assert L.lpipm_k_iteration(cx._h, C.byref(_opts()), 0, p(x), p(y), p(z), C.byref(one), C.byref(one), p(np.empty(n)),
                               p(np.empty(m)), p(np.empty(n)), p(tk), C.byref(one), None) == _capi.ERR_UNSUPPORTED
    # the refused calls left the batch as it was
    cx.upload_lockstep_shared_ub_tall(X, bs, cs)
    assert L.lpipm_k_adat(cx._h, p(d), p(M), 1, None) == _capi.ERR_UNSUPPORTED
    _assert_members(cx.solve_lockstep(_opts()), SMALL, specs, (), "after the refusals")
    cx.close()


class _NeverCalled:
    """An all-reduce for lpipm_set_collective that no refused upload may reach."""
    def __init__(self):
        from lp_amd import _capi
        self.calls = 0
        self.cfn = _capi.ALLREDUCE_FN(self._call)

    def _call(self, *args):
        self.calls += 1
        return 1


def _raw_upload(cx, count, X, bs, cs):
    from lp_amd import _capi
    dp = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    arr = lambda lst: (dp * len(lst))(*[p(a) for a in lst])
    return _capi.lib().lpipm_upload_lockstep_shared_ub_tall(cx._h, count, X.shape[1], X.shape[0], p(X), X.shape[1], arr(bs), arr(cs), None)


def test_refused_on_a_column_split_context_and_above_4096_members(built):
    import lp_amd
    from lp_amd import _capi
    X = np.ascontiguousarray(_X(SMALL))
    bs, cs = [[np.ascontiguousarray(a) for a in v] for v in _vectors(SMALL, _specs(3))]
    cx = lp_amd.Context(0)
    coll = _NeverCalled()
    cx.set_collective(1, 2, coll)                                    # one rank of a column split over two
    assert _raw_upload(cx, 3, X, bs, cs) == _capi.ERR_UNSUPPORTED
    assert cx.resident_bytes() == 0 and coll.calls == 0              # nothing resident, nothing reduced
    with pytest.raises(lp_amd.BackendError):
        cx.upload_lockstep_shared_ub_tall(X, bs, cs)
    cx.set_collective(0, 1, None)                                    # the same context without the split takes the batch
    assert _raw_upload(cx, 4097, X, bs * 1366, cs * 1366) == _capi.ERR_BAD_ARGUMENT      # the member count's bound
    assert cx.resident_bytes() == 0
    assert _raw_upload(cx, 3, X, bs, cs) == _capi.OK
    cx._lock = (3, SMALL[0], SMALL[0] + SMALL[1], None, bs, cs)
    _assert_members(cx.solve_lockstep(_opts()), SMALL, _specs(3), (), "after the refusals")
    cx.close()


def test_refused_on_a_refining_context(built, monkeypatch):
    """The refined solves are switched on from the environment when a context is created (behind the library's master switch)."""
    import lp_amd
    from lp_amd import _capi
    X = np.ascontiguousarray(_X(SMALL))
    bs, cs = [[np.ascontiguousarray(a) for a in v] for v in _vectors(SMALL, _specs(3))]
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_REFINE", "2")
    cx = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_REFINE")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    assert _raw_upload(cx, 3, X, bs, cs) == _capi.ERR_UNSUPPORTED
    assert cx.resident_bytes() == 0
    b, c = _member(SMALL, 0)                                         # as the single tall upload on such a context
    with pytest.raises(lp_amd.BackendError):
        cx.upload(lp_amd.Problem.target(c).ub(X, b).build(), tall=True)
    cx.close()
