"""The first iteration's factor, kept per upload: every solve starts from x = z = 1, so iteration 1's normal matrix,
its Cholesky factor, the block inverses and the pivot-failure word are functions of A alone, and every solve after the first on
one upload starts from the kept ones.  Nothing may change by a bit: every comparison here is exact, and the reference is
always a fresh context with the switch off (lpipm_set_first_factor_cache(ctx, 0))."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _assert_same(got, ref, what):
    """(status, x, fun, iterations, log rows) of solve_raw: equal status and count, x and fun bit for bit, every row of the log."""
    assert got[0] == ref[0] and got[3] == ref[3], (what, got[0], ref[0], got[3], ref[3])
    assert _bits(got[1]) == _bits(ref[1]), what
    if got[1] is not None and not np.isnan(ref[1]).any():
        assert np.array_equal(got[1], ref[1]), what
    assert _bits(got[2]) == _bits(ref[2]), (what, got[2], ref[2])
    assert len(got[4]) == len(ref[4]) and _bits(np.array(got[4])) == _bits(np.array(ref[4])), what


def _assert_same_members(got, ref, what):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and g[3] == r[3], (what, i, g[0], r[0], g[3], r[3])
        assert _bits(g[1]) == _bits(r[1]) and _bits(g[2]) == _bits(r[2]), (what, i)


def _off_context():
    import lp_amd
    return lp_amd.Context(0).set_first_factor_cache(False)


def _reference(upload, opts):
    ref = _off_context()
    upload(ref)
    out = ref.solve_raw(opts, want_log=True)
    ref.close()
    return out


def _ub_eq_lp(seed, nx, m_ub, m_eq):
    """min c.x st A_ub x <= b_ub, A_eq x = b_eq, x >= 0: feasible (x0 > 0 is strictly inside) and bounded (A_ub > 0)."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(0.1, 1.0, nx)
    A_ub = rng.uniform(0.0, 1.0, (m_ub, nx)); b_ub = A_ub @ x0 + rng.uniform(0.5, 1.0, m_ub)
    A_eq = rng.standard_normal((m_eq, nx)); b_eq = A_eq @ x0
    return A_ub, b_ub, A_eq, b_eq, rng.standard_normal(nx)


# ---- repeat solves ----------------------------------------------------------------------------------------------------------
# 200x450: the fused small-LP vector stage, whose starting residual launch does iteration 1's pred_setup; 1100x2300: the
# unfused stage, mp = 1152 (a partial last super-block); 1536x3072 with the look-ahead forced: iteration 1 of the first solve
# factors into the kept buffers with the predictor beside the chain, the kept iteration of later solves runs the serial order
@pytest.mark.parametrize("m,n,force", [(200, 450, False), (1100, 2300, False), (1536, 3072, True)])
def test_repeat_solves_equal_the_uncached_solve(built, monkeypatch, m, n, force):
    import lp_amd
    from lp_amd import synth
    if force:
        monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
        monkeypatch.setenv("LPIPM_LOOKAHEAD", "1")
    A, b, c, _ = synth.planted_lp(3, m, n)
    o = _opts()
    ref = _reference(lambda cx: cx.upload_arrays(A, b, c), o)
    assert ref[0] == 0 and ref[3] > 2
    ctx = lp_amd.Context(0)
    ctx.upload_arrays(A, b, c)
    for k in range(3):
        _assert_same(ctx.solve_raw(o, want_log=True), ref, f"solve {k + 1}")
    ctx.close()


@pytest.mark.parametrize("form", ["upload_slack", "upload_ub_eq"])
def test_repeat_solves_with_a_structural_slack_block(built, form):
    """The slack rows' diagonal of iteration 1 (+ I) is part of what is kept."""
    import lp_amd
    A_ub, b_ub, A_eq, b_eq, c = _ub_eq_lp(11, 300, 260, 90)
    prob = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build()
    if form == "upload_ub_eq":
        up = lambda cx: cx.upload(prob)
    else:
        up = lambda cx: cx.upload_arrays(prob.A(), prob.b(), prob.c(), prob.c0(), prob.n_slack())
    o = _opts()
    ref = _reference(up, o)
    assert ref[0] == 0
    ctx = lp_amd.Context(0)
    up(ctx)
    for k in range(3):
        _assert_same(ctx.solve_raw(o, want_log=True), ref, f"{form} solve {k + 1}")
    ctx.close()


# ---- options changed between solves -------------------------------------------------------------------------------------------
def test_options_changed_between_solves(built):
    """The kept factor depends on none of them: each solve equals the uncached solve with the same options."""
    import lp_amd
    from lp_amd import synth, _capi
    A, b, c, _ = synth.planted_lp(5, 300, 700)
    variants = [dict(), dict(ip=0), dict(tol=1e-6), dict(max_iter=1), dict(ip=0, max_iter=2), dict(max_iter=2), dict(ip=1)]
    ctx = lp_amd.Context(0)
    ctx.upload_arrays(A, b, c)
    for kw in variants:
        o = _opts(**kw)
        ref = _reference(lambda cx: cx.upload_arrays(A, b, c), o)
        got = ctx.solve_raw(o, want_log=True)
        _assert_same(got, ref, str(kw))
        if "max_iter" in kw:     # the iteration limit comes with its x
            assert got[0] == _capi.ITERATION_LIMIT and got[3] == kw["max_iter"] and not np.isnan(got[1]).any()
    ctx.close()


# ---- invalidation --------------------------------------------------------------------------------------------------------------
def test_reupload_of_the_same_geometry_drops_the_kept_factor(built):
    import lp_amd
    from lp_amd import synth
    A0, b0, c0, _ = synth.planted_lp(1, 260, 600)
    A1, b1, c1, _ = synth.planted_lp(2, 260, 600)
    o = _opts()
    ref = _reference(lambda cx: cx.upload_arrays(A1, b1, c1), o)
    ctx = lp_amd.Context(0)
    ctx.upload_arrays(A0, b0, c0)
    assert ctx.solve_raw(o)[0] == 0
    assert ctx.solve_raw(o)[0] == 0
    ctx.upload_arrays(A1, b1, c1)                 # the arena stays; what it kept belongs to A0
    _assert_same(ctx.solve_raw(o, want_log=True), ref, "first solve on the second matrix")
    _assert_same(ctx.solve_raw(o, want_log=True), ref, "second solve on the second matrix")
    ctx.close()


def test_single_lockstep_single_drops_the_kept_factor(built):
    import lp_amd
    from lp_amd import synth
    lps = [synth.planted_lp(20 + k, 200, 450)[:3] for k in range(4)]
    o = _opts()
    ctx = lp_amd.Context(0)
    ctx.upload_arrays(*lps[0])
    first = ctx.solve_raw(o, want_log=True)
    _assert_same(ctx.solve_raw(o, want_log=True), first, "single, second solve")
    ctx.upload_lockstep([p[0] for p in lps[1:]], [p[1] for p in lps[1:]], [p[2] for p in lps[1:]])
    batch = ctx.solve_lockstep(o)
    _assert_same_members(ctx.solve_lockstep(o), batch, "lockstep, second solve")
    ctx.upload_arrays(*lps[3])
    got = [ctx.solve_raw(o, want_log=True), ctx.solve_raw(o, want_log=True)]
    ctx.close()
    ref = _reference(lambda cx: cx.upload_arrays(*lps[3]), o)
    for k, g in enumerate(got):
        _assert_same(g, ref, f"single again, solve {k + 1}")
    assert batch[2][0] == ref[0] and batch[2][3] == ref[3] and _bits(batch[2][1]) == _bits(ref[1])   # and as a batch member
    _assert_same(first, _reference(lambda cx: cx.upload_arrays(*lps[0]), o), "the first single LP")


# ---- update_vectors ------------------------------------------------------------------------------------------------------------
def test_update_vectors_equals_a_fresh_upload(built):
    import lp_amd
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(7, 260, 600)
    _, b2, c2, _ = synth.planted_lp(8, 260, 600)
    rng = np.random.default_rng(0)
    x2 = np.where(rng.uniform(size=600) < 0.4, rng.uniform(1.0, 2.0, 600), 0.0)
    b2 = A @ x2                                    # feasible for A
    c2 = np.abs(c2) + 0.1                          # bounded below on x >= 0
    o = _opts()
    ref = _reference(lambda cx: cx.upload_arrays(A, b2, c2), o)
    assert ref[0] == 0
    ctx = lp_amd.Context(0)
    ctx.upload_arrays(A, b, c)
    assert ctx.solve_raw(o)[0] == 0
    ctx.update_vectors(b2, c2)
    _assert_same(ctx.solve_raw(o, want_log=True), ref, "after update_vectors")
    ctx.update_vectors(b, c)
    _assert_same(ctx.solve_raw(o, want_log=True), _reference(lambda cx: cx.upload_arrays(A, b, c), o), "and back")
    ctx.close()


def test_update_vectors_error_returns(built):
    import lp_amd
    from lp_amd import synth, _capi
    L = _capi.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    A, b, c, _ = synth.planted_lp(0, 64, 150)
    ctx = lp_amd.Context(0)
    assert L.lpipm_update_vectors(ctx._h, dp(b), dp(c)) == _capi.ERR_NO_PROBLEM
    ctx.upload_arrays(A, b, c)
    assert L.lpipm_update_vectors(ctx._h, None, dp(c)) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_vectors(ctx._h, dp(b), dp(c)) == _capi.OK
    A_ub, b_ub, A_eq, b_eq, cx = _ub_eq_lp(1, 40, 30, 10)
    ctx.upload(lp_amd.Problem.target(cx).ub(A_ub, b_ub).eq(A_eq, b_eq).build())          # lpipm_upload_ub_eq
    bb, cc = np.zeros(40), np.zeros(70)
    assert L.lpipm_update_vectors(ctx._h, dp(bb), dp(cc)) == _capi.ERR_UNSUPPORTED
    ctx.upload_lockstep([A, A], [b, b], [c, c])
    assert L.lpipm_update_vectors(ctx._h, dp(b), dp(c)) == _capi.ERR_UNSUPPORTED
    ctx.set_collective(0, 1, None)
    ctx.upload_column_block(A, b, c, A.shape[1])
    assert L.lpipm_update_vectors(ctx._h, dp(b), dp(c)) == _capi.ERR_UNSUPPORTED
    ctx.close()


# ---- a kept pivot failure ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", ["two identical rows", "a zero row"])
def test_rank_deficient_matrix_fails_on_every_solve(built, defect):
    """A.A^T of a rank-deficient A has a non-positive pivot: the kept word is replayed, every solve is NumericalProblem."""
    import lp_amd
    from lp_amd import synth, _capi
    A, b, c, _ = synth.planted_lp(4, 64, 150)
    if defect == "two identical rows":
        A[1] = A[0]; b[1] = b[0]
    else:
        A[5] = 0.0; b[5] = 0.0
    o = _opts()
    ref = _reference(lambda cx: cx.upload_arrays(A, b, c), o)
    assert ref[0] == _capi.NUMERICAL_PROBLEM
    ctx = lp_amd.Context(0)
    ctx.upload_arrays(A, b, c)
    for k in range(3):
        _assert_same(ctx.solve_raw(o, want_log=True), ref, f"{defect}, solve {k + 1}")
    ctx.close()


# ---- lockstep batches ----------------------------------------------------------------------------------------------------------
def _scaled_members(count, m, n, seed):
    """Planted LPs whose costs differ in scale, so that the members stop at different iterations."""
    from lp_amd import synth
    out = []
    for k in range(count):
        A, b, c, _ = synth.planted_lp(seed + k, m, n)
        out.append((A, b * (1.0 + 3.0 * (k % 3)), c * 10.0 ** (k % 4)))
    return out


def _lockstep_case(upload, o, want_spread=True):
    import lp_amd
    ref = _off_context()
    upload(ref)
    want = ref.solve_lockstep(o)
    ref.close()
    ctx = lp_amd.Context(0)
    upload(ctx)
    first = ctx.solve_lockstep(o)
    second = ctx.solve_lockstep(o)
    third = ctx.solve_lockstep(o)
    ctx.close()
    _assert_same_members(first, want, "first solve")
    _assert_same_members(second, want, "second solve")
    _assert_same_members(third, want, "third solve")
    its = sorted({w[3] for w in want})
    print(f"\n[measure] iterations of the members {[w[3] for w in want]}")
    assert all(w[0] == 0 for w in want)
    if want_spread:
        assert len(its) > 1, its           # some members stop earlier than others


def test_lockstep_members_with_their_own_matrix(built):
    lps = _scaled_members(4, 200, 450, 40)
    _lockstep_case(lambda cx: cx.upload_lockstep([p[0] for p in lps], [p[1] for p in lps], [p[2] for p in lps]), _opts())


def test_lockstep_half_batch_views(built):
    """18 members run as two half-batch views of 9: the validity lives with the parent."""
    lps = _scaled_members(18, 128, 300, 60)
    _lockstep_case(lambda cx: cx.upload_lockstep([p[0] for p in lps], [p[1] for p in lps], [p[2] for p in lps]), _opts())


def test_lockstep_members_on_a_shared_matrix(built):
    from lp_amd import synth
    A = synth.planted_lp(80, 200, 450)[0]
    rng = np.random.default_rng(80)
    bs, cs = [], []
    for k in range(6):
        x = np.where(rng.uniform(size=450) < 0.4, rng.uniform(1.0, 2.0, 450), 0.0)
        bs.append(A @ x * (1.0 + 3.0 * (k % 3)))
        cs.append(rng.uniform(0.1, 2.0, 450) * 10.0 ** (k % 4))
    _lockstep_case(lambda cx: cx.upload_lockstep_shared(A, bs, cs), _opts())


# ---- the arms that do not use it -----------------------------------------------------------------------------------------------
def test_qr_arm_is_unchanged(built):
    import lp_amd
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(9, 130, 300)
    o = _opts(solver_type=int(lp_amd.EquationSolverType.LeastSquares))
    ref = _reference(lambda cx: cx.upload_arrays(A, b, c), o)
    assert ref[0] == 0
    ctx = lp_amd.Context(0)
    ctx.upload_arrays(A, b, c)
    chol = ctx.solve_raw(_opts(), want_log=True)           # a Cholesky solve first: something is kept
    for k in range(2):
        _assert_same(ctx.solve_raw(o, want_log=True), ref, f"QR solve {k + 1}")
    _assert_same(ctx.solve_raw(_opts(), want_log=True), chol, "Cholesky again, behind the QR solves")
    ctx.close()


class _ThreadRanks:
    """The all-reduce of lpipm_set_collective for `world` ranks that are threads of this process, each with its own
    context on the one device (drained contract): every rank publishes its operand, rank 0 reduces them in rank order, every
    rank copies the result.  A rank that never arrives breaks the barrier for all instead of leaving them waiting."""

    def __init__(self, world):
        self.world, self.barrier = world, threading.Barrier(world, timeout=60)
        self.ops, self.result = [None] * world, None

    def rank(self, r):
        return _ThreadRank(self, r)


class _ThreadRank:
    on_stream = False

    def __init__(self, ranks, r):
        from lp_amd import _capi
        self.g, self.r, self.calls, self.error = ranks, r, 0, None
        self.cfn = _capi.ALLREDUCE_FN(self._call)

    def _call(self, _user, ptr, count, op, _stream):
        try:
            import torch
            from lp_amd.colsplit import _DevPtr
            g = self.g
            t = torch.as_tensor(_DevPtr(ptr, count), device=torch.device("cuda", 0))
            g.ops[self.r] = t
            g.barrier.wait()
            if self.r == 0:
                acc = g.ops[0].clone()
                for other in g.ops[1:]:
                    acc = torch.minimum(acc, other) if op == 1 else acc + other
                g.result = acc
                torch.cuda.synchronize()
            g.barrier.wait()
            t.copy_(g.result)
            torch.cuda.synchronize()
            g.barrier.wait()
            self.calls += 1
            return 0
        except Exception as e:      # never unwind through the C frames
            self.error = e
            return 1


def _solve_on_thread_ranks(A, b, c, o, cache_on, solves):
    import lp_amd
    from lp_amd.colsplit import column_range
    world, n = 2, A.shape[1]
    ranks = _ThreadRanks(world)
    out = [None] * world

    def run(r):
        cols = column_range(n, world, r)
        ctx = lp_amd.Context(0).set_first_factor_cache(cache_on)
        coll = ranks.rank(r)
        ctx.set_collective(r, world, coll)
        ctx.upload_column_block(np.ascontiguousarray(A[:, cols.start:cols.stop]), b, c[cols.start:cols.stop], n)
        got = []
        for _ in range(solves):
            before = coll.calls
            res = ctx.solve_raw(o, want_log=True)
            got.append((res, coll.calls - before))
        ctx.close()
        out[r] = (got, coll.error)

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
        assert not t.is_alive()
    for got, err in out:
        assert err is None, err
    return [got for got, _ in out]


def test_column_split_is_unchanged(built):
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(0, 256, 512)
    o = _opts()
    ref = _solve_on_thread_ranks(A, b, c, o, False, 1)
    got = _solve_on_thread_ranks(A, b, c, o, True, 2)
    for r in range(2):
        (first, calls1), (second, calls2) = got[r]
        assert first[0] == 0 and calls1 > 0
        _assert_same(first, ref[r][0][0], f"rank {r}, first solve")
        _assert_same(second, ref[r][0][0], f"rank {r}, second solve")
        assert calls2 == calls1 == ref[r][0][1]          # every reduction of every iteration is still made


# ---- counters and memory -------------------------------------------------------------------------------------------------------
def test_adat_launches_are_the_launches_made(built):
    import lp_amd
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(3, 300, 700)
    o = _opts()
    ref = _reference(lambda cx: cx.upload_arrays(A, b, c), o)
    for mode in (1, 2):
        ctx = lp_amd.Context(0)
        ctx.set_profiling(mode)
        ctx.upload_arrays(A, b, c)
        seen = []
        for k in range(3):
            _assert_same(ctx.solve_raw(o, want_log=True), ref, f"profiling {mode}, solve {k + 1}")
            seen.append(ctx.phase_times())
        ctx.close()
        its = ref[3]
        assert [t["iterations"] for t in seen] == [its] * 3
        assert [t["adat_launches"] for t in seen] == [its, its - 1, its - 1], seen
        assert all(t["adat_ms"] > 0.0 for t in seen)
        if mode == 1:
            assert all(t["potrf_ms"] > 0.0 for t in seen)
    off = _off_context()
    off.set_profiling(1)
    off.upload_arrays(A, b, c)
    for _ in range(2):
        off.solve_raw(o)
        assert off.phase_times()["adat_launches"] == off.phase_times()["iterations"] == ref[3]
    off.close()


def _kept_bytes(m):
    """include/lpipm.h, lpipm_set_first_factor_cache: 8 mp^2 + 16 sum s_k^2 + 4096 per resident LP."""
    mp = -(-m // 128) * 128
    w = 512 if mp <= 2048 else 1024
    return 8 * mp * mp + 16 * sum(min(w, mp - r0) ** 2 for r0 in range(0, mp, w)) + 4096


@pytest.mark.parametrize("m,n,count", [(200, 450, 1), (1100, 2300, 1), (2100, 2200, 1), (128, 300, 18)])
def test_resident_bytes_count_the_kept_factor(built, m, n, count):
    import lp_amd
    rng = np.random.default_rng(0)
    A, b, c = rng.standard_normal((m, n)), rng.standard_normal(m), rng.standard_normal(n)
    got = {}
    for on in (True, False):
        ctx = lp_amd.Context(0).set_first_factor_cache(on)
        if count == 1:
            ctx.upload_arrays(A, b, c)
        else:
            ctx.upload_lockstep([A] * count, [b] * count, [c] * count)
        got[on] = ctx.resident_bytes()
        if not on:             # switched on for a resident problem: the buffers come with the next upload
            ctx.set_first_factor_cache(True)
            assert ctx.resident_bytes() == got[False]
            ctx.upload_arrays(A, b, c)
            got["again"] = ctx.resident_bytes()
        ctx.close()
    assert got[True] - got[False] == count * _kept_bytes(m), (got, _kept_bytes(m))
    if count == 1:
        assert got["again"] == got[True]
