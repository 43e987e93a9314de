"""Power-of-two row and column equilibration of the resident matrix (lpipm_set_scaling).  The factors are powers of
two, so scaling and unscaling are exact: the exponents equal the numpy restatement of the rule below exactly, and a solve with
scaling on is bit-identical to an ordinary solve, on a fresh context that never heard of scaling, of the same LP scaled on the
host with those exponents.  Only `test_it_helps` compares with a tolerance (the planted optimum, 1e-6)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- the rule, restated ----------------------------------------------------------------------------------------------------------
def rule(X, passes, n_slack=0):
    """-> (kr[m], kc[nx + n_slack]) for the structural block X (m x nx); slack column i gets -kr[i]."""
    kr, kc = np.zeros(X.shape[0], dtype=np.int32), np.zeros(X.shape[1], dtype=np.int32)

    def step(a):
        f, e = np.frexp(a)
        return np.where(np.isfinite(a) & (a > 0), -(e // 2), 0).astype(np.int32)
    for _ in range(passes):
        S = np.abs(np.ldexp(X, kr[:, None] + kc[None, :]))
        rmax, cmax = np.fmax.reduce(S, axis=1, initial=0.0), np.fmax.reduce(S, axis=0, initial=0.0)
        kr, kc = kr + step(rmax), kc + step(cmax)
    return kr, np.concatenate([kc, -kr[:n_slack]])


def scaled(A, b, c, kr, kc):
    return np.ldexp(A, kr[:, None] + kc[None, :]), np.ldexp(b, kr), np.ldexp(c, kc)


def disturbed(seed, m, n, s=16):
    """A planted LP whose rows and columns are multiplied by 2^U{-s..s}: (A, b, c) of the disturbed problem, the planted
    optimum x* of the undisturbed one and the columns' exponents ec (the disturbed optimum is ldexp(x*, -ec))."""
    from lp_amd import synth
    A, b, c, xs = synth.planted_lp(seed, m, n)
    rng = np.random.default_rng(1000 + seed)
    er, ec = rng.integers(-s, s + 1, m).astype(np.int32), rng.integers(-s, s + 1, n).astype(np.int32)
    A, b, c = scaled(A, b, c, er, ec)
    return A, b, c, xs, ec


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _new(passes=0, cache=True):
    import lp_amd
    return lp_amd.Context(0).set_first_factor_cache(cache).set_scaling(passes)


def _assert_scaled_same(got, ref, kc, what):
    """solve_raw of the scaling context against solve_raw of the host-scaled LP: status, count, every log row and fun bit for
    bit; x = ldexp(x_ref, kc) bit for bit (None on both sides without a solution)."""
    assert got[0] == ref[0] and got[3] == ref[3], (what, got[0], ref[0], got[3], ref[3])
    assert (got[1] is None) == (ref[1] is None), what
    if ref[1] is not None and not np.isnan(ref[1]).any():
        assert _bits(got[1]) == _bits(np.ldexp(ref[1], kc)), what
    else:
        assert _bits(got[1]) == _bits(ref[1]), what
    assert _bits(got[2]) == _bits(ref[2]), (what, got[2], ref[2])
    assert len(got[4]) == len(ref[4]) and _bits(np.array(got[4])) == _bits(np.array(ref[4])), what


def _assert_member_same(g, r, kc, what):
    """(status, x, fun, iterations) of a batch member against solve_raw of its host-scaled single solve."""
    assert g[0] == r[0] and g[3] == r[3], (what, g[0], r[0], g[3], r[3])
    if r[0] in (0, 7):
        assert _bits(g[1]) == _bits(np.ldexp(r[1], kc)) and _bits(g[2]) == _bits(r[2]), what
    else:
        assert g[1] is None, what


def _plain_solve(up, o, want_log=True):
    """solve_raw on a fresh context with scaling off and nothing kept."""
    ref = _new(0, cache=False)
    up(ref)
    out = ref.solve_raw(o, want_log=want_log)
    ref.close()
    return out


def _ub_eq_lp(seed, nx, m_ub, m_eq, s=12):
    """tests/test_gpu_first_factor_cache.py's inequality-form LP (feasible, bounded), rows and columns disturbed by 2^U{-s..s}."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(0.1, 1.0, nx)
    A_ub = rng.uniform(0.0, 1.0, (m_ub, nx)); b_ub = A_ub @ x0 + rng.uniform(0.5, 1.0, m_ub)
    A_eq = rng.standard_normal((m_eq, nx)); b_eq = A_eq @ x0
    c = rng.standard_normal(nx)
    eu, ee, ec = (rng.integers(-s, s + 1, k).astype(np.int32) for k in (m_ub, m_eq, nx))
    return (np.ldexp(A_ub, eu[:, None] + ec[None, :]), np.ldexp(b_ub, eu), np.ldexp(A_eq, ee[:, None] + ec[None, :]),
            np.ldexp(b_eq, ee), np.ldexp(c, ec))


# ---- 1. exponents ------------------------------------------------------------------------------------------------------------------
def _matrix(seed, m, n):
    rng = np.random.default_rng(seed)
    e = rng.integers(-16, 17, m)[:, None] + rng.integers(-16, 17, n)[None, :]
    return np.ldexp(rng.standard_normal((m, n)), e), rng.standard_normal(m), rng.standard_normal(n)


# (129, 17) and (1100, 2300): n no multiple of 16, m no multiple of 128 -- padding lanes beside live ones in both directions;
# (1100, 2300) has five column chunks and nine row blocks
@pytest.mark.parametrize("passes", [1, 8])
@pytest.mark.parametrize("m,n", [(1, 1), (5, 9), (129, 17), (200, 450), (1100, 2300)])
def test_exponents_equal_the_rule(built, m, n, passes):
    A, b, c = _matrix(m * 7 + n, m, n)
    ctx = _new(passes)
    ctx.upload_arrays(A, b, c)
    kr, kc = ctx.scaling()
    ctx.close()
    wr, wc = rule(A, passes)
    assert kr.dtype == np.int32 and np.array_equal(kr, wr) and np.array_equal(kc, wc)
    assert np.abs(wr).max() > 0 or m == 1


def test_exponents_with_a_leading_dimension(built):
    """lda > n: what lies between the rows is neither copied nor looked at."""
    from lp_amd import _capi
    m, n, lda = 131, 277, 300
    A, b, c = _matrix(5, m, n)
    wide = np.full((m, lda), 2.0 ** 40)
    wide[:, :n] = A
    ctx = _new(8)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert _capi.lib().lpipm_upload(ctx._h, m, n, dp(wide), lda, dp(b), dp(c), 0.0) == 0
    ctx.m, ctx.n = m, n
    kr, kc = ctx.scaling()
    ctx.close()
    wr, wc = rule(A, 8)
    assert np.array_equal(kr, wr) and np.array_equal(kc, wc)


@pytest.mark.parametrize("passes", [1, 8])
def test_exponents_zero_row_zero_column_and_inf(built, passes):
    """A row and a column of zeros keep exponent 0; a row / column whose maximum is inf does not move either."""
    m, n = 140, 530
    A, b, c = _matrix(9, m, n)
    A[7, :] = 0.0
    A[:, 513] = 0.0
    A[100, 20] = np.inf
    ctx = _new(passes)
    ctx.upload_arrays(A, b, c)
    kr, kc = ctx.scaling()
    ctx.close()
    wr, wc = rule(A, passes)
    assert np.array_equal(kr, wr) and np.array_equal(kc, wc)
    assert kr[7] == 0 and kc[513] == 0 and kr[100] == 0 and kc[20] == 0


def test_scaling_before_an_upload_and_when_off(built):
    import lp_amd
    from lp_amd import _capi
    ctx = lp_amd.Context(0)
    ctx.m, ctx.n = 3, 4
    with pytest.raises(lp_amd.BackendError):
        ctx.scaling()                                   # LPIPM_ERR_NO_PROBLEM
    A, b, c = _matrix(1, 20, 50)
    ctx.upload_arrays(A, b, c)
    kr, kc = ctx.scaling()
    assert not kr.any() and not kc.any() and kr.shape == (20,) and kc.shape == (50,)
    e = (C.c_int32 * 64)()
    assert _capi.lib().lpipm_get_scaling(ctx._h, 1, e, e) == _capi.ERR_BAD_ARGUMENT     # one member is resident
    ctx.close()


# ---- 2. bit-identity, single LP ----------------------------------------------------------------------------------------------------
# (200, 450): the fused vector stage; (1100, 2300): the unfused one, several column chunks and row blocks of the maxima pass
@pytest.mark.parametrize("m,n,kw", [(200, 450, {}), (1100, 2300, {}), (200, 450, dict(max_iter=3))])
def test_single_lp_equals_the_host_scaled_solve(built, m, n, kw):
    from lp_amd import _capi
    A, b, c, _, _ = disturbed(3, m, n)
    o = _opts(**kw)
    kr, kc = rule(A, 8)
    As, bs, cs = scaled(A, b, c, kr, kc)
    ref = _plain_solve(lambda cx: cx.upload_arrays(As, bs, cs), o)
    ctx = _new(8)
    ctx.upload_arrays(A, b, c)
    dr, dc = ctx.scaling()
    assert np.array_equal(dr, kr) and np.array_equal(dc, kc)
    for k in range(2):                                   # the second solve starts from the kept factor of the scaled matrix
        _assert_scaled_same(ctx.solve_raw(o, want_log=True), ref, kc, f"solve {k + 1}")
    ctx.close()
    if kw:
        assert ref[0] == _capi.ITERATION_LIMIT and ref[3] == 3 and not np.isnan(ref[1]).any()
    else:
        assert ref[0] == 0


def test_single_lp_without_a_solution(built):
    from lp_amd import _capi
    A = np.array([[1.0, -1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]])          # unbounded (tests/test_gpu_lockstep.py)
    b, c = np.array([0.0, 1.0]), np.array([-1.0, 0.0, 0.0, 0.0])
    er, ec = np.array([9, -7], dtype=np.int32), np.array([3, -11, 6, 0], dtype=np.int32)
    A, b, c = scaled(A, b, c, er, ec)
    kr, kc = rule(A, 8)
    As, bs, cs = scaled(A, b, c, kr, kc)
    o = _opts()
    ref = _plain_solve(lambda cx: cx.upload_arrays(As, bs, cs), o)
    ctx = _new(8)
    ctx.upload_arrays(A, b, c)
    got = ctx.solve_raw(o, want_log=True)
    ctx.close()
    assert ref[0] in (_capi.INFEASIBLE, _capi.UNBOUNDED)
    assert got[0] == ref[0] and got[3] == ref[3] and _bits(np.array(got[4])) == _bits(np.array(ref[4]))
    assert np.isnan(got[1]).all()                        # x_out untouched


def test_qr_arm_sees_the_scaled_matrix(built):
    A, b, c, _, _ = disturbed(4, 60, 150)
    kr, kc = rule(A, 8)
    As, bs, cs = scaled(A, b, c, kr, kc)
    o = _opts(solver_type=1)
    ref = _plain_solve(lambda cx: cx.upload_arrays(As, bs, cs), o)
    ctx = _new(8)
    ctx.upload_arrays(A, b, c)
    _assert_scaled_same(ctx.solve_raw(o, want_log=True), ref, kc, "inverse arm")
    ctx.close()
    assert ref[0] == 0


def test_device_destination_is_unscaled(built):
    import torch
    A, b, c, _, _ = disturbed(5, 200, 450)
    o = _opts()
    ctx = _new(8)
    ctx.upload_arrays(A, b, c)
    host = ctx.solve_raw(o)
    xd = torch.zeros(450, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = ctx.solve_raw(o, x_dev_ptr=xd.data_ptr())
    ctx.close()
    assert host[0] == 0 and dev[0] == 0 and _bits(xd.cpu().numpy()) == _bits(host[1])


# ---- 3. structural slack -------------------------------------------------------------------------------------------------------------
def test_structural_slack_paths(built):
    import lp_amd
    nx, m_ub, m_eq = 70, 40, 20
    A_ub, b_ub, A_eq, b_eq, c = _ub_eq_lp(11, nx, m_ub, m_eq)
    prob = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build()
    A, b, cs = prob.A(), prob.b(), prob.c()
    o = _opts()
    # the two structural paths: the rule on the m x nx block, slack exponents -kr
    kr, kc = rule(A[:, :nx], 8, n_slack=m_ub)
    assert np.array_equal(kc[nx:], -kr[:m_ub])
    As, bs, css = scaled(A, b, cs, kr, kc)
    assert np.array_equal(As[:, nx:], A[:, nx:])          # [I; 0] stays [I; 0]
    ref = _plain_solve(lambda cx: cx.upload_arrays(As, bs, css, 0.0, m_ub), o)
    assert ref[0] == 0
    outs = []
    for name, up in (("upload, hint verified", lambda cx: cx.upload_arrays(A, b, cs, 0.0, m_ub)),
                     ("upload_ub_eq", lambda cx: cx.upload(prob))):
        ctx = _new(8)
        up(ctx)
        dr, dc = ctx.scaling()
        assert np.array_equal(dr, kr) and np.array_equal(dc, kc), name
        got = ctx.solve_raw(o, want_log=True)
        ctx.close()
        _assert_scaled_same(got, ref, kc, name)
        outs.append(got)
    assert _bits(outs[0][1]) == _bits(outs[1][1])
    # the explicit dense slack-form matrix, hint off: the plain rule on all columns
    kr_d, kc_d = rule(A, 8)
    Ad, bd, cd = scaled(A, b, cs, kr_d, kc_d)
    ref_d = _plain_solve(lambda cx: cx.upload_arrays(Ad, bd, cd), o)
    ctx = _new(8)
    ctx.upload_arrays(A, b, cs)
    dr, dc = ctx.scaling()
    assert np.array_equal(dr, kr_d) and np.array_equal(dc, kc_d)
    _assert_scaled_same(ctx.solve_raw(o, want_log=True), ref_d, kc_d, "dense slack form")
    ctx.close()


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------------
def test_lockstep_members_own_their_exponents(built):
    m, n = 130, 300
    lps = [disturbed(s, m, n)[:3] for s in (0, 1, 2)]
    o = _opts()
    ctx = _new(8)
    ctx.upload_lockstep([p[0] for p in lps], [p[1] for p in lps], [p[2] for p in lps])
    exps = [ctx.scaling(i) for i in range(3)]
    res = ctx.solve_lockstep(o)
    ctx.close()
    for i, (A, b, c) in enumerate(lps):
        kr, kc = rule(A, 8)
        assert np.array_equal(exps[i][0], kr) and np.array_equal(exps[i][1], kc), i
        As, bs, cs = scaled(A, b, c, kr, kc)
        ref = _plain_solve(lambda cx: cx.upload_arrays(As, bs, cs), o, want_log=False)
        assert ref[0] == 0
        _assert_member_same(res[i], ref, kc, f"member {i}")
    assert not np.array_equal(exps[0][0], exps[1][0])


def test_lockstep_in_two_half_batch_views(built):
    """17 members: solved as two views (8 and 9 members) on two streams, each unscaling its own rows with its own exponents."""
    m, n, K = 24, 60, 17
    lps = [disturbed(s, m, n)[:3] for s in range(K)]
    o = _opts()
    ctx = _new(8)
    ctx.upload_lockstep([p[0] for p in lps], [p[1] for p in lps], [p[2] for p in lps])
    res = ctx.solve_lockstep(o)
    exps = [ctx.scaling(i) for i in (0, 8, 16)]
    ctx.close()
    for k, i in enumerate((0, 8, 16)):
        kr, kc = rule(lps[i][0], 8)
        assert np.array_equal(exps[k][0], kr) and np.array_equal(exps[k][1], kc), i
    single = _new(8, cache=False)
    for i, (A, b, c) in enumerate(lps):
        single.upload_arrays(A, b, c)
        r = single.solve_raw(o)
        assert res[i][0] == r[0] and res[i][3] == r[3], i
        if r[0] == 0:
            assert _bits(res[i][1]) == _bits(r[1]) and _bits(res[i][2]) == _bits(r[2]), i
    single.close()
    assert sum(r[0] == 0 for r in res) >= K // 2


def test_shared_matrix_batch_has_one_set(built):
    """Five members: a short last group of the 4-wide shared template."""
    m, n = 130, 300
    A, b, c, _, _ = disturbed(6, m, n)
    rng = np.random.default_rng(0)
    bs = [b * (1.0 + 0.1 * rng.random(m)) if i else b for i in range(5)]
    cs = [c * (1.0 + 0.1 * rng.random(n)) if i else c for i in range(5)]
    o = _opts()
    kr, kc = rule(A, 8)
    ctx = _new(8)
    ctx.upload_lockstep_shared(A, bs, cs)
    dr, dc = ctx.scaling()
    assert np.array_equal(dr, kr) and np.array_equal(dc, kc)
    res = ctx.solve_lockstep(o)
    ctx.close()
    for i in range(5):
        As, b_s, c_s = scaled(A, bs[i], cs[i], kr, kc)
        ref = _plain_solve(lambda cx: cx.upload_arrays(As, b_s, c_s), o, want_log=False)
        _assert_member_same(res[i], ref, kc, f"member {i}")
    assert res[0][0] == 0


def test_shared_ub_eq_batch(built):
    import lp_amd
    nx, m_ub, m_eq = 70, 40, 20
    A_ub, b_ub, A_eq, b_eq, c = _ub_eq_lp(12, nx, m_ub, m_eq)
    rng = np.random.default_rng(1)
    bs = [np.concatenate([b_ub * (1.0 + 0.05 * rng.random(m_ub)), b_eq]) for _ in range(5)]
    cs = [c * (1.0 + 0.05 * rng.random(nx)) for _ in range(5)]
    prob = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build()
    A = prob.A()
    kr, kc = rule(A[:, :nx], 8, n_slack=m_ub)
    o = _opts()
    ctx = _new(8)
    ctx.upload_lockstep_shared_ub_eq(A_ub, A_eq, bs, cs)
    dr, dc = ctx.scaling()
    assert np.array_equal(dr, kr) and np.array_equal(dc, kc)
    res = ctx.solve_lockstep(o)
    ctx.close()
    for i in range(5):
        As, b_s, c_s = scaled(A, bs[i], np.concatenate([cs[i], np.zeros(m_ub)]), kr, kc)
        ref = _plain_solve(lambda cx: cx.upload_arrays(As, b_s, c_s, 0.0, m_ub), o, want_log=False)
        _assert_member_same(res[i], ref, kc, f"member {i}")
    assert res[0][0] == 0


def test_solve_batch_of_two_shapes(built):
    """Two members of one shape go through a lockstep group, the two odd ones through the one-by-one path, one of them on a
    worker context: the switch reaches all of them."""
    lps = [disturbed(0, 130, 300)[:3], disturbed(1, 130, 300)[:3], disturbed(2, 60, 150)[:3], disturbed(3, 70, 160)[:3]]
    o = _opts()
    ctx = _new(8)
    res = ctx.solve_batch([(A, b, c, 0.0) for A, b, c in lps], o)
    ctx.close()
    for i, (A, b, c) in enumerate(lps):
        kr, kc = rule(A, 8)
        As, bs, cs = scaled(A, b, c, kr, kc)
        ref = _plain_solve(lambda cx: cx.upload_arrays(As, bs, cs), o, want_log=False)
        assert ref[0] == 0
        _assert_member_same(res[i], ref, kc, f"member {i}")


# ---- 5. vector updates and the kept factor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", [True, False])
def test_update_vectors_uses_the_kept_exponents(built, cache):
    m, n = 200, 450
    A, b, c, _, _ = disturbed(7, m, n)
    rng = np.random.default_rng(2)
    b2, c2 = b * (1.0 + 0.1 * rng.random(m)), c * (1.0 + 0.1 * rng.random(n))
    o = _opts()
    fresh = _new(8, cache=False)
    fresh.upload_arrays(A, b2, c2)
    ref = fresh.solve_raw(o, want_log=True)
    fresh.close()
    ctx = _new(8, cache=cache)
    ctx.upload_arrays(A, b, c)
    assert ctx.solve_raw(o)[0] == 0                      # (with the cache on: leaves the scaled matrix's first factor behind)
    ctx.update_vectors(b2, c2)
    got = ctx.solve_raw(o, want_log=True)
    ctx.close()
    assert ref[0] == 0 and got[0] == ref[0] and got[3] == ref[3]
    assert _bits(got[1]) == _bits(ref[1]) and _bits(got[2]) == _bits(ref[2]) and _bits(np.array(got[4])) == _bits(np.array(ref[4]))


@pytest.mark.parametrize("device", [False, True])
def test_update_lockstep_vectors_on_a_shared_batch(built, device):
    import torch
    m, n, K = 130, 300, 5
    A, b, c, _, _ = disturbed(8, m, n)
    rng = np.random.default_rng(3)
    bs = [b * (1.0 + 0.1 * rng.random(m)) for _ in range(K)]
    cs = [c * (1.0 + 0.1 * rng.random(n)) for _ in range(K)]
    bs2 = [b * (1.0 + 0.1 * rng.random(m)) for _ in range(K)]
    cs2 = [c * (1.0 + 0.1 * rng.random(n)) for _ in range(K)]
    o = _opts()
    fresh = _new(8)
    fresh.upload_lockstep_shared(A, bs2, cs2)
    ref = fresh.solve_lockstep(o)
    fresh.close()
    ctx = _new(8)
    ctx.upload_lockstep_shared(A, bs, cs)
    assert ctx.solve_lockstep(o)[0][0] == 0
    if device:
        bd = torch.tensor(np.stack(bs2), dtype=torch.float64, device="cuda")
        cd = torch.tensor(np.stack(cs2), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.update_lockstep_vectors_device(bd.data_ptr(), m, cd.data_ptr(), n)
    else:
        ctx.update_lockstep_vectors(bs2, cs2)
    got = ctx.solve_lockstep(o)
    # only b replaced: c keeps its scaled values and is not scaled twice
    ctx.update_lockstep_vectors(bs, None)
    got_b = ctx.solve_lockstep(o)
    ctx.close()
    fresh = _new(8)
    fresh.upload_lockstep_shared(A, bs, cs2)
    ref_b = fresh.solve_lockstep(o)
    fresh.close()
    for i in range(K):
        for g, r in ((got[i], ref[i]), (got_b[i], ref_b[i])):
            assert g[0] == r[0] == 0 and g[3] == r[3] and _bits(g[1]) == _bits(r[1]) and _bits(g[2]) == _bits(r[2]), i


# ---- 6. off means off ------------------------------------------------------------------------------------------------------------------
def test_off_means_off(built):
    import lp_amd
    A, b, c, _, _ = disturbed(9, 200, 450, s=4)
    o = _opts()
    never = lp_amd.Context(0)
    never.upload_arrays(A, b, c)
    ref = never.solve_raw(o, want_log=True)
    ref_bytes = never.resident_bytes()
    never.close()
    ctx = _new(8)
    ctx.upload_arrays(A, b, c)
    assert ctx.resident_bytes() > ref_bytes              # the exponents and the slabs are counted while they exist
    ctx.set_scaling(0)
    ctx.upload_arrays(A, b, c)
    kr, kc = ctx.scaling()
    got = ctx.solve_raw(o, want_log=True)
    assert not kr.any() and not kc.any() and ctx.resident_bytes() == ref_bytes
    ctx.close()
    assert got[0] == ref[0] and got[3] == ref[3] and _bits(got[1]) == _bits(ref[1]) and _bits(got[2]) == _bits(ref[2])
    assert _bits(np.array(got[4])) == _bits(np.array(ref[4]))


# ---- 7. it helps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_it_helps(built, seed):
    """130x300 planted LP, rows and columns disturbed by 2^U{-16..16}: with 8 passes the device is Optimal in at most half the
    iterations the CPU oracle takes on the same input without scaling (measured on the oracle alone: 36-39 against 8), and x,
    mapped back to the undisturbed units, agrees with the planted optimum to 1e-6."""
    from oracle import capi as oracle
    m, n = 130, 300
    A, b, c, xs, ec = disturbed(seed, m, n)
    base = oracle.solve(A, b, c, want_log=False)
    ctx = _new(8)
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, _ = ctx.solve_raw(_opts())
    ctx.close()
    print(f"seed {seed}: oracle unscaled status {base['status']} in {base['iterations']} iterations, device scaled {rc} in {it}")
    assert rc == 0 and 2 * it <= base["iterations"], (rc, it, base["iterations"])
    err = np.abs(np.ldexp(x, ec) - xs).max()             # both in the undisturbed LP's units
    print(f"seed {seed}: max |x - x*| = {err:.3e}")
    assert err <= 1e-6


def test_passes_out_of_range_on_a_context(built):
    """-1 and 65 are refused and leave the switch as it was; 64 is accepted."""
    from lp_amd import _capi
    A, b, c = _matrix(2, 20, 50)
    ctx = _new(1)
    assert _capi.lib().lpipm_set_scaling(ctx._h, -1) == _capi.ERR_BAD_ARGUMENT
    assert _capi.lib().lpipm_set_scaling(ctx._h, 65) == _capi.ERR_BAD_ARGUMENT
    ctx.upload_arrays(A, b, c)
    kr, kc = ctx.scaling()
    wr, wc = rule(A, 1)
    assert np.array_equal(kr, wr) and np.array_equal(kc, wc)
    ctx.set_scaling(64).upload_arrays(A, b, c)
    kr, kc = ctx.scaling()
    ctx.close()
    wr, wc = rule(A, 64)
    assert np.array_equal(kr, wr) and np.array_equal(kc, wc)


# ---- 8. refused ----------------------------------------------------------------------------------------------------------------------------
def test_column_split_upload_is_refused(built):
    import lp_amd
    from lp_amd import _capi
    A, b, c, _, _ = disturbed(0, 60, 150)
    ctx = _new(8)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert _capi.lib().lpipm_upload_nsplit(ctx._h, 60, 150, 150, dp(A), 150, dp(b), dp(c), 0.0) == _capi.ERR_UNSUPPORTED
    with pytest.raises(lp_amd.BackendError):
        ctx.upload_column_block(A, b, c, 150)
    ctx.set_scaling(0)
    ctx.upload_column_block(A, b, c, 150)                # world = 1: an ordinary upload through the column-split entry
    ctx.close()
