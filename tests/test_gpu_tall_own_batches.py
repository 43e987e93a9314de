"""Lockstep batches of tall inequality-form LPs whose members own their matrices (lpipm_upload_lockstep_ub_tall,
lpipm_solve_batch_ub_tall).

The yardstick is the single tall solve: every member of a batch -- whatever the count, wherever it sits, whichever members
have already stopped, as one view or two half-batch views, through the upload entry or the batch entry, at every max_group --
has the status, iteration count, fun and the bytes of x of Context.upload(problem, tall=True) + solve_raw of that member alone.
Besides: the oracle on the slack form, new vectors in place, scaling with exponents per member, memory, geometry switches on
one context and the refusals.

Shapes as in tests/test_gpu_tall_batches.py: (300, 40) -- mp 384, mk 304, npa 48, nxp 128, no multiple of any tile -- and
(1100, 130) -- mp 1152, nxp 256 (two diagonal blocks of K), npa 144; (4100, 650) is the shape whose single LP builds K on the
round-2 kernel.  Counts 1, 3 (a short group), 8 (the XCD-major A.D.A^T grid), 11 (8 + 3) and 19 (two views of 9 and 10)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-6                     # the tall form's own bound against the oracle (tests/test_gpu_tall_form.py)
SMALL, LARGE, TINY = (300, 40), (1100, 130), (64, 8)
PLAIN, INF, UNB = "plain", "infeasible", "unbounded"


# ---- generator --------------------------------------------------------------------------------------------------------------------
def own_X(seed, m, nx):          # row 0 >= 0 and column 0 <= 0: lets a member be made infeasible or unbounded
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    X[0, :] = np.abs(X[0, :])
    X[:, 0] = -np.abs(X[:, 0])
    X[0, 0] = 0.0
    return X


def member(X, seed):             # exactly as in tests/test_gpu_tall_batches.py
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
def _X(shape, i):
    X = own_X(7000 + 37 * shape[0] + i, *shape)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _member(shape, spec):
    """spec = (i, kind[, vectors]): matrix i of the shape with the vectors of member `vectors` (default i), made infeasible
    (b[0] = -1) or unbounded (c[0] = -1) by its kind.  -> b, c"""
    i, kind = spec[0], spec[1]
    j = spec[2] if len(spec) > 2 else i
    b, c = member(_X(shape, i), 1000 * shape[0] + j)
    if kind == INF:
        b[0] = -1.0              # row 0 of X is >= 0 and x >= 0
    if kind == UNB:
        c[0] = -1.0              # column 0 of X is <= 0
    b.setflags(write=False); c.setflags(write=False)
    return b, c


def _specs(count, shift=0):
    """Members 0 .. count - 1; from count 3 on member 1 is infeasible and the last one unbounded (in a batch of 19: one in each
    half).  shift: the vectors are those of members i + shift, on the matrices of members i."""
    kind = lambda i: INF if count >= 3 and i == 1 else UNB if count >= 3 and i == count - 1 else PLAIN
    return [(i, kind(i), i + shift) if shift else (i, kind(i)) for i in range(count)]


def _arrays(shape, specs):
    ms = [_member(shape, s) for s in specs]
    return [_X(shape, s[0]) for s in specs], [m[0] for m in ms], [m[1] for m in ms]


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


def _problem(shape, spec):
    import lp_amd
    b, c = _member(shape, spec)
    return lp_amd.Problem.target(c).ub(_X(shape, spec[0]), b).build()


@functools.lru_cache(maxsize=None)
def _single(shape, spec, kw=()):
    """The single tall solve of one member: computed once per (member, options), shared, immutable."""
    import lp_amd
    cx = lp_amd.Context(0)
    cx.upload(_problem(shape, spec), tall=True)
    rc, x, fun, it, _ = cx.solve_raw(_opts(**dict(kw)))
    cx.close()
    return _norm(rc, x, fun, it)


def _assert_members(res, shapes, specs, kw=(), what=""):
    """shapes: one shape for all members, or a list of one per member."""
    if isinstance(shapes, tuple):
        shapes = [shapes] * len(specs)
    assert len(res) == len(specs)
    for pos, (shape, spec, r) in enumerate(zip(shapes, specs, res)):
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
    ctx.upload_lockstep_ub_tall(*_arrays(shape, specs))
    assert (ctx.m, ctx.n) == (shape[0], shape[0] + shape[1])
    res = ctx.solve_lockstep(_opts(**dict(kw)))
    _assert_members(res, shape, specs, kw, f"{shape} x {count} {kw}")
    if dict(kw).get("max_iter") == 3:
        for spec, r in zip(specs, res):
            if spec[1] == PLAIN:
                assert r[0] == 7 and r[3] == 3 and not np.isnan(r[1]).any()          # IterationLimit, x filled
    else:
        assert sorted({r[0] for r in res}) == ([0, 5, 6] if count >= 3 else [0])
    again = ctx.solve_lockstep(_opts(**dict(kw)))                                     # and again on the same upload
    assert [_norm(*r) for r in again] == [_norm(*r) for r in res]


# ---- 2. different matrices, the same vectors --------------------------------------------------------------------------------------
def test_two_matrices_with_the_same_vectors(ctx):
    """A zero member stride on X or on Xt would solve member 0's LP twice."""
    import lp_amd
    b, c = _member(SMALL, (0, PLAIN))
    Xs = [_X(SMALL, 0), _X(SMALL, 1)]
    ctx.upload_lockstep_ub_tall(Xs, [b, b], [c, c])
    res = [_norm(*r) for r in ctx.solve_lockstep(_opts(max_iter=5))]
    one = lp_amd.Context(0)
    for X, got in zip(Xs, res):
        one.upload(lp_amd.Problem.target(c).ub(X, b).build(), tall=True)
        assert got == _norm(*one.solve_raw(_opts(max_iter=5))[:4])
    one.close()
    assert res[0][1] is not None and res[0][1] != res[1][1]


# ---- 3. the round-2 plan ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [2, 8, 17], ids=["2", "8-xcd-major", "17-two-views"])
def test_a_plan_that_a_single_lp_runs_on_the_round2_kernel(built, count):
    """nxp = 768 (21 tiles of K) and 257 k-tiles: the single LP's K comes from the round-2 kernel, whose bits depend on its
    workgroup count -- every member of the batch runs that very plan on its own Xt, also on the XCD-major grid (count 8) and
    under half-batch views (count 17).  Two distinct members repeat: only two single solves are needed."""
    import lp_amd
    shape = (4100, 650)
    specs = [(i % 2, PLAIN) for i in range(count)]
    cx = lp_amd.Context(0)
    cx.upload_lockstep_ub_tall(*_arrays(shape, specs))
    res = cx.solve_lockstep(_opts(max_iter=4))
    cx.close()
    _assert_members(res, shape, specs, (("max_iter", 4),), "round-2 plan")


# ---- 4. against the oracle ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(shape, spec):
    from oracle import capi as oracle
    X = _X(shape, spec[0])
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
    ctx.upload_lockstep_ub_tall(*_arrays(SMALL, specs))
    res = ctx.solve_lockstep(_opts())
    assert [r[0] for r in res] == [0, 5, 0, 0, 0, 0, 0, 6]
    _check_oracle(SMALL, specs, res)


def test_two_large_members_against_the_oracle(ctx):
    specs = _specs(5)
    ctx.upload_lockstep_ub_tall(*_arrays(LARGE, specs))
    res = ctx.solve_lockstep(_opts())
    _check_oracle(LARGE, [specs[0], specs[2]], [res[0], res[2]])


# ---- 5. lpipm_solve_batch_ub_tall on a mixed list ----------------------------------------------------------------------------------
def _mixed():
    """Seven (300, 40) -- member 1 infeasible, member 6 unbounded --, two (1100, 130) and one (64, 8), interleaved."""
    small = [(SMALL, s) for s in _specs(7)]
    large = [(LARGE, (0, PLAIN)), (LARGE, (2, PLAIN))]
    order = small[:2] + large[:1] + small[2:5] + [(TINY, (0, PLAIN))] + small[5:] + large[1:]
    return [o[0] for o in order], [o[1] for o in order]


@pytest.mark.parametrize("max_group", [-1, 0, 3])
def test_solve_batch_on_a_mixed_list(built, max_group):
    import lp_amd
    import torch
    from lp_amd import _capi
    shapes, specs = _mixed()
    problems = [_problem(sh, sp) for sh, sp in zip(shapes, specs)]
    cx = lp_amd.Context(0)
    assert _capi.lib().lpipm_set_batch_lockstep(cx._h, max_group) == _capi.OK
    res = cx.solve_batch(problems, _opts(), tall=True)
    _assert_members(res, shapes, specs, (), f"host rows, max_group {max_group}")
    assert sorted({r[0] for r in res}) == [0, 5, 6]
    # the device block: rows longer than the longest x, the sentinel stays wherever no x goes
    stride = max(m + nx for m, nx in shapes) + 5
    dev = torch.device("cuda", 0)
    rows = torch.full((len(problems), stride), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    resd = cx.solve_batch_device(problems, _opts(), rows.data_ptr(), stride, tall=True)
    got = rows.cpu().numpy()
    for i, ((rc, x, fun, it), (rcd, fund, itd)) in enumerate(zip(res, resd)):
        assert (rc, it) == (rcd, itd) and _bits(fun) == _bits(fund), i
        n = sum(shapes[i])
        if x is None:
            assert np.all(got[i] == -7.0), i
        else:
            assert _bits(got[i, :n]) == _bits(x) and np.all(got[i, n:] == -7.0), i
    with pytest.raises(lp_amd.BackendError):
        cx.solve_batch_device(problems, _opts(), rows.data_ptr(), stride - 6, tall=True)      # shorter than the longest x
    cx.close()


def test_solve_batch_member_without_rows_is_unconstrained(built):
    """Member 1 has m_ub = 0: its status is LPIPM_UNCONSTRAINED, the call returns Ok and the others are solved."""
    import lp_amd
    from lp_amd import _capi
    dp = C.POINTER(C.c_double)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(dp)
    specs = [(0, PLAIN), None, (1, PLAIN), (2, PLAIN)]
    m, nx = SMALL
    As, bs, cs = [], [], []
    for s in specs:
        b, c = _member(SMALL, s) if s else (np.zeros(1), np.ones(nx))
        As.append(np.ascontiguousarray(_X(SMALL, s[0])) if s else np.zeros((1, nx)))
        bs.append(np.ascontiguousarray(b)); cs.append(np.ascontiguousarray(c))
    K = len(specs)
    arr = lambda lst: (dp * K)(*[p(a) for a in lst])
    xs = [np.full(m + nx, np.nan) for _ in range(K)]
    mu = (C.c_uint64 * K)(*[m if s else 0 for s in specs]); n = (C.c_uint64 * K)(*[nx] * K)
    fun = (C.c_double * K)(); its = (C.c_uint64 * K)(); st = (C.c_int32 * K)()
    cx = lp_amd.Context(0)
    L = _capi.lib()
    o = _opts()
    rc = L.lpipm_solve_batch_ub_tall(cx._h, K, mu, n, arr(As), arr(bs), arr(cs), None, C.byref(o), arr(xs), None, 0, fun, its, st)
    assert rc == _capi.OK and st[1] == _capi.UNCONSTRAINED
    keep = [i for i, s in enumerate(specs) if s]
    _assert_members([(st[i], xs[i], fun[i], its[i]) for i in keep], SMALL, [specs[i] for i in keep], (), "beside m_ub = 0")
    # exactly one of the host rows and the device block
    assert L.lpipm_solve_batch_ub_tall(cx._h, K, mu, n, arr(As), arr(bs), arr(cs), None, C.byref(o), None, None, 0, fun, its, st) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_solve_batch_ub_tall(cx._h, K, mu, n, arr(As), arr(bs), arr(cs), None, C.byref(o), arr(xs), C.c_void_p(8), m + nx,
                                       fun, its, st) == _capi.ERR_BAD_ARGUMENT
    cx.close()


# ---- 6. new vectors in place ---------------------------------------------------------------------------------------------------------
def test_update_lockstep_vectors(built):
    import lp_amd
    import torch
    o = _opts()
    old, new = _specs(8), _specs(8, shift=100)        # the vectors of members i + 100 on the matrices of members i
    (Xs, b0, c0), (_, b1, c1) = _arrays(SMALL, old), _arrays(SMALL, new)

    def fresh(bs, cs):
        f = lp_amd.Context(0)
        f.upload_lockstep_ub_tall(Xs, bs, cs)
        out = [_norm(*r) for r in f.solve_lockstep(o)]
        f.close()
        return out

    cx = lp_amd.Context(0)
    cx.upload_lockstep_ub_tall(Xs, b0, c0)
    _assert_members(cx.solve_lockstep(o), SMALL, old, (), "first upload")
    cx.update_lockstep_vectors(bs=b1)                                               # b alone
    assert [_norm(*r) for r in cx.solve_lockstep(o)] == fresh(b1, c0)
    cx.update_lockstep_vectors(b1, c1)                                              # the host variant
    res = cx.solve_lockstep(o)
    assert [_norm(*r) for r in res] == fresh(b1, c1)
    _assert_members(res, SMALL, new, (), "b and c replaced")
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        cx.update_lockstep_vectors(cs=[np.zeros(SMALL[0] + SMALL[1])] * 8)          # the lockstep form: the n structural costs
    # the device variant: packed row blocks on the device, rows longer than the vectors
    m, nx = SMALL
    ldb, ldc = m + 5, nx + 3
    hb, hc = np.full((8, ldb), np.nan), np.full((8, ldc), np.nan)
    hb[:, :m], hc[:, :nx] = np.array(b0), np.array(c0)
    dev = torch.device("cuda", 0)
    tb, tc = torch.from_numpy(hb).to(dev), torch.from_numpy(hc).to(dev)
    torch.cuda.synchronize(dev)
    cx.update_lockstep_vectors_device(tb.data_ptr(), ldb, tc.data_ptr(), ldc)
    _assert_members(cx.solve_lockstep(o), SMALL, old, (), "device blocks")
    cx.close()


# ---- 7. scaling ----------------------------------------------------------------------------------------------------------------------
def test_scaling_keeps_exponents_per_member(built):
    import lp_amd
    m, nx = SMALL
    rng = np.random.default_rng(7)
    specs = _specs(8)
    Xs, bs, cs = _arrays(SMALL, specs)
    Xd, bd, cd = [], [], []
    for X, b, c in zip(Xs, bs, cs):                   # every member disturbed by its own powers of two
        er, ec = rng.integers(-8, 9, m), rng.integers(-8, 9, nx)
        Xd.append(np.ldexp(X, er[:, None] + ec[None, :])); bd.append(np.ldexp(b, er)); cd.append(np.ldexp(c, ec))
    o = _opts()
    cx = lp_amd.Context(0).set_scaling(8)
    cx.upload_lockstep_ub_tall(Xd, bd, cd)
    exps = [cx.scaling(i) for i in range(8)]
    res = [_norm(*r) for r in cx.solve_lockstep(o)]
    assert any(not np.array_equal(exps[0][0], e[0]) for e in exps[1:]) and any(not np.array_equal(exps[0][1], e[1]) for e in exps[1:])
    one = lp_amd.Context(0).set_scaling(8)
    for i in range(8):
        one.upload(lp_amd.Problem.target(cd[i]).ub(Xd[i], bd[i]).build(), tall=True)
        kr1, kc1 = one.scaling()
        assert np.array_equal(exps[i][0], kr1) and np.array_equal(exps[i][1], kc1), i
        rc, x, fun, it, _ = one.solve_raw(o)
        assert res[i] == _norm(rc, x, fun, it), (i, res[i][0], rc, res[i][3], it)
    # ... and later vectors are scaled with the kept exponents
    cx.update_lockstep_vectors(bd, cd)
    assert [_norm(*r) for r in cx.solve_lockstep(o)] == res
    one.close(); cx.close()


# ---- 8. memory -----------------------------------------------------------------------------------------------------------------------
def test_resident_bytes_do_not_grow_as_m_squared(built):
    import lp_amd

    def resident(shape):
        cx = lp_amd.Context(0)
        cx.upload_lockstep_ub_tall([_X(shape, i) for i in range(8)], [np.ones(shape[0])] * 8, [np.ones(shape[1])] * 8)
        out = cx.resident_bytes()
        cx.close()
        return out

    once, twice = resident((300, 40)), resident((600, 40))
    print(f"\n[measure] resident bytes of 8 members: m = 300: {once}, m = 600: {twice} ({twice / once:.2f} x)")
    assert twice < 2.5 * once, (once, twice)          # an m^2 term would make it about 4 x


# ---- 9. geometry switches on one context ------------------------------------------------------------------------------------------------
def test_geometry_switches(built):
    """single tall -> owned batch -> shared tall batch -> dense -> owned batch, on one context."""
    import lp_amd
    from lp_amd import synth
    specs = _specs(3)
    Xs, bs, cs = _arrays(SMALL, specs)
    cx = lp_amd.Context(0)
    cx.upload(_problem(SMALL, specs[0]), tall=True)
    assert _norm(*cx.solve_raw(_opts())[:4]) == _single(SMALL, specs[0])
    cx.upload_lockstep_ub_tall(Xs, bs, cs)
    _assert_members(cx.solve_lockstep(_opts()), SMALL, specs, (), "owned batch after a single tall LP")
    # the shared batch over member 0's matrix: its member k is (X_0, vectors of member k)
    shared = [(0, PLAIN, 0), (0, PLAIN, 2), (0, PLAIN, 3)]
    vs = [_member(SMALL, s) for s in shared]
    cx.upload_lockstep_shared_ub_tall(_X(SMALL, 0), [v[0] for v in vs], [v[1] for v in vs])
    _assert_members(cx.solve_lockstep(_opts()), SMALL, shared, (), "shared batch after an owned one")
    A, b2, c2, _ = synth.planted_lp(3, 64, 160)
    fresh = lp_amd.Context(0)
    fresh.upload_arrays(A, b2, c2)
    want = _norm(*fresh.solve_raw(_opts())[:4])
    fresh.close()
    cx.upload_arrays(A, b2, c2)
    assert _norm(*cx.solve_raw(_opts())[:4]) == want and want[0] == 0
    cx.upload_lockstep_ub_tall(Xs, bs, cs)
    _assert_members(cx.solve_lockstep(_opts()), SMALL, specs, (), "owned batch after a dense LP")
    cx.close()


# ---- 10. refusals and codes -----------------------------------------------------------------------------------------------------------
def _contig(shape, specs):
    Xs, bs, cs = _arrays(shape, specs)
    return [np.ascontiguousarray(a) for a in Xs], [np.ascontiguousarray(a) for a in bs], [np.ascontiguousarray(a) for a in cs]


def _raw_upload(cx, count, Xs, bs, cs, lda=None):
    from lp_amd import _capi
    dp = C.POINTER(C.c_double)
    arr = lambda lst: (dp * len(lst))(*[a.ctypes.data_as(dp) for a in lst])
    m, nx = Xs[0].shape
    return _capi.lib().lpipm_upload_lockstep_ub_tall(cx._h, count, nx, m, arr(Xs), nx if lda is None else lda, arr(bs), arr(cs), None)


def test_refusals_and_codes(built):
    import lp_amd
    from lp_amd import _capi
    L = _capi.lib()
    dp = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)
    m, nx = SMALL
    specs = _specs(3)
    Xs, bs, cs = _contig(SMALL, specs)
    arr = lambda lst: (dp * len(lst))(*[p(a) for a in lst])
    cx = lp_amd.Context(0)
    up = L.lpipm_upload_lockstep_ub_tall
    assert up(cx._h, 3, nx, 0, arr(Xs), nx, arr(bs), arr(cs), None) == _capi.UNCONSTRAINED
    assert up(cx._h, 0, nx, m, arr(Xs), nx, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, None, nx, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, arr(Xs), nx, None, arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, arr(Xs), nx, arr(bs), None, None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, arr(Xs), nx - 1, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, (dp * 3)(p(Xs[0]), None, p(Xs[2])), nx, arr(bs), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert up(cx._h, 3, nx, m, arr(Xs), nx, (dp * 3)(p(bs[0]), None, p(bs[2])), arr(cs), None) == _capi.ERR_BAD_ARGUMENT
    assert _raw_upload(cx, 4097, Xs * 1366, bs * 1366, cs * 1366) == _capi.ERR_BAD_ARGUMENT           # the member count's bound
    assert cx.resident_bytes() == 0
    cx.upload_lockstep_ub_tall(Xs, bs, cs)
    for st in (1, 2):
        with pytest.raises(lp_amd.BackendError):
            cx.solve_lockstep(_opts(solver_type=st))
        held = [np.empty(m + nx) for _ in range(3)]
        xs = (dp * 3)(*[p(a) for a in held])
        assert L.lpipm_solve_lockstep(cx._h, C.byref(_opts(solver_type=st)), xs, None, None, (C.c_int32 * 3)()) == _capi.ERR_UNSUPPORTED
    n = m + nx
    d, K, M = np.ones(n), np.empty((nx, nx)), np.empty((m, m))
    x, y, z, tk = np.ones(n), np.ones(m), np.ones(n), np.ones(2)
    one = C.c_double(1.0)

    def refused_kernel_entries():
        U, V = np.empty(n), np.empty(m)
        assert L.lpipm_k_tall_normal(cx._h, p(d), p(K)) == _capi.ERR_UNSUPPORTED
        assert L.lpipm_k_tall_sym_solve(cx._h, p(d), 1, p(np.ones(n)), p(np.ones(m)), p(U), p(V), None) == _capi.ERR_UNSUPPORTED
        assert L.lpipm_k_adat(cx._h, p(d), p(M), 1, None) == _capi.ERR_UNSUPPORTED
        assert L.lpipm_k_iteration(cx._h, C.byref(_opts()), 0, p(x), p(y), p(z), C.byref(one), C.byref(one), p(np.empty(n)),
                                   p(np.empty(m)), p(np.empty(n)), p(tk), C.byref(one), None) == _capi.ERR_UNSUPPORTED

    refused_kernel_entries()
    cx.upload_lockstep_ub_tall(Xs[:1], bs[:1], cs[:1])                 # a batch of ONE is a batch too
    refused_kernel_entries()
    cx.upload_lockstep_ub_tall(Xs, bs, cs)                             # the refused calls leave a batch as it was
    refused_kernel_entries()
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


def test_refused_on_a_column_split_context(built):
    import lp_amd
    from lp_amd import _capi
    specs = _specs(3)
    Xs, bs, cs = _contig(SMALL, specs)
    cx = lp_amd.Context(0)
    coll = _NeverCalled()
    cx.set_collective(1, 2, coll)                                    # one rank of a column split over two
    assert _raw_upload(cx, 3, Xs, bs, cs) == _capi.ERR_UNSUPPORTED
    assert cx.resident_bytes() == 0 and coll.calls == 0              # nothing resident, nothing reduced
    cx.set_collective(0, 1, None)                                    # the same context without the split takes the batch
    cx.upload_lockstep_ub_tall(Xs, bs, cs)
    _assert_members(cx.solve_lockstep(_opts()), SMALL, specs, (), "after the refusal")
    cx.close()


def test_refused_on_a_refining_context(built, monkeypatch):
    """The refined solves are switched on from the environment when a context is created (behind the library's master switch)."""
    import lp_amd
    from lp_amd import _capi
    Xs, bs, cs = _contig(SMALL, _specs(3))
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_REFINE", "2")
    cx = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_REFINE")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    assert _raw_upload(cx, 3, Xs, bs, cs) == _capi.ERR_UNSUPPORTED
    assert cx.resident_bytes() == 0
    cx.close()
