"""New b, c and c0 in place for a resident lockstep batch (lpipm_update_lockstep_vectors[_device]), the ONE kept first factor
of a shared-matrix batch and the sweep drivers on top of them (lp_amd.batch.sweep_shared_*).

Every comparison is exact -- status, iteration count, the bytes of x and fun -- and the reference side is always the path
that existed before: a fresh context with the first-factor cache off, a fresh upload_lockstep* of the same members and
solve_lockstep.  The shapes are the smallest that reach each path:
  200 x 450, 6 members    one super-block; one full and one short group of 4, a short group of 8
  1100 x 2300             mp = 1152: super-blocks 512, 512, 128, so the factor's panel updates and transposed panel products
                          exist; 5 members = 2 groups, 640 rows x 2 <= 2048: one row per wave; 13 members = 4 groups: four
                          rows per wave with a row tail
  128 x 300, 18 members   two half-batch views of 9"""
import ctypes as C
import functools

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


def _assert_same_members(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[0] == r[0] and g[3] == r[3], (what, i, g[0], r[0], g[3], r[3])
        assert _bits(g[1]) == _bits(r[1]) and _bits(g[2]) == _bits(r[2]), (what, i)


def _off_context():
    import lp_amd
    return lp_amd.Context(0).set_first_factor_cache(False)


def _fresh(upload, o=None, want_ok=True, want_spread=True):
    """The reference: a fresh context with the cache off, a fresh upload, solve_lockstep."""
    ref = _off_context()
    upload(ref)
    want = ref.solve_lockstep(o or _opts())
    ref.close()
    print(f"\n[measure] iterations of the reference members {[w[3] for w in want]}")
    if want_ok:
        assert all(w[0] == 0 for w in want), [w[0] for w in want]
    if want_spread:
        assert len({w[3] for w in want}) > 1, [w[3] for w in want]       # some members stop earlier than others
    return want


@functools.lru_cache(maxsize=None)
def _shared_sets(seed, m, n, count, nsets=2):
    """One planted A and `nsets` sets of `count` members on it: b = A x (x >= 0, sparse), c > 0, both scaled per member so
    that the members stop at different iterations; every set with constants of its own.  -> (A, [(bs, cs, c0s), ...])"""
    from lp_amd import synth
    A = synth.planted_lp(seed, m, n)[0]
    rng = np.random.default_rng(seed)
    sets = []
    for _ in range(nsets):
        bs, cs = [], []
        for k in range(count):
            x = np.where(rng.uniform(size=n) < 0.4, rng.uniform(1.0, 2.0, n), 0.0)
            bs.append(A @ x * (1.0 + 3.0 * (k % 3)))
            cs.append(rng.uniform(0.1, 2.0, n) * 10.0 ** (k % 4))
        sets.append((bs, cs, [float(v) for v in rng.uniform(-2.0, 2.0, count)]))
    return A, sets


@functools.lru_cache(maxsize=None)
def _shared_ref(seed, m, n, count, which):
    A, sets = _shared_sets(seed, m, n, count)
    bs, cs, c0s = sets[which]
    return _fresh(lambda cx: cx.upload_lockstep_shared(A, bs, cs, c0s))


# ---- 1: update equals fresh upload, one super-block ---------------------------------------------------------------------------
def test_update_equals_fresh_upload_one_superblock(built):
    import lp_amd
    seed, m, n, count = 80, 200, 450, 6
    A, (s0, s1) = _shared_sets(seed, m, n, count)
    want0, want1 = _shared_ref(seed, m, n, count, 0), _shared_ref(seed, m, n, count, 1)
    o = _opts()
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, *s0)
    _assert_same_members(ctx.solve_lockstep(o), want0, "set 0, first solve")
    ctx.update_lockstep_vectors(*s1)
    _assert_same_members(ctx.solve_lockstep(o), want1, "set 1 after the update")
    _assert_same_members(ctx.solve_lockstep(o), want1, "set 1, second solve")
    ctx.update_lockstep_vectors(*s0)
    _assert_same_members(ctx.solve_lockstep(o), want0, "back to set 0")
    ctx.close()
    # one member of set 1 alone, through the single-LP path
    k = 4
    one = _off_context()
    one.upload_arrays(A, s1[0][k], s1[1][k], s1[2][k])
    rc, x, fun, it, _ = one.solve_raw(o)
    one.close()
    assert (rc, it) == (want1[k][0], want1[k][3]) and _bits(x) == _bits(want1[k][1]) and _bits(fun) == _bits(want1[k][2])


# ---- 2, 3: the factor's panels through the shared templates ---------------------------------------------------------------------
@pytest.mark.parametrize("count", [5, 13])
def test_factor_panels_through_the_shared_templates(built, count):
    """mp = 1152: 640 rows below the first super-block.  5 members: 2 groups of 4, one row per wave; 13 members: 4 groups, four
    rows per wave; 2 groups of 8 for the transposed panel products either way, the last one short."""
    import lp_amd
    seed, m, n = 90 + count, 1100, 2300
    A, (s0, s1) = _shared_sets(seed, m, n, count)
    want0, want1 = _shared_ref(seed, m, n, count, 0), _shared_ref(seed, m, n, count, 1)
    o = _opts()
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, *s0)
    _assert_same_members(ctx.solve_lockstep(o), want0, "first solve")
    _assert_same_members(ctx.solve_lockstep(o), want0, "second solve")
    ctx.update_lockstep_vectors(*s1)
    _assert_same_members(ctx.solve_lockstep(o), want1, "after the update")
    ctx.close()


# ---- 4: two half-batch views ------------------------------------------------------------------------------------------------------
def test_two_half_batch_views(built):
    """18 members run as two views of 9 on two host threads: the one factor is built before both are dispatched."""
    import lp_amd
    seed, m, n, count = 60, 128, 300, 18
    A, (s0, s1) = _shared_sets(seed, m, n, count)
    want0, want1 = _shared_ref(seed, m, n, count, 0), _shared_ref(seed, m, n, count, 1)
    o = _opts()
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, *s0)
    _assert_same_members(ctx.solve_lockstep(o), want0, "first solve")
    _assert_same_members(ctx.solve_lockstep(o), want0, "second solve")
    ctx.update_lockstep_vectors(*s1)
    _assert_same_members(ctx.solve_lockstep(o), want1, "after the update")
    ctx.close()


# ---- 5: structural slack forms ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _slack_family(count=4, nx=150, m_ub=70, m_eq=30, nsets=2):
    """The scenario family of tests/test_gpu_slack_batches.py: A_ub, A_eq ~ N(0,1) once; per member x0 ~ U(0.5, 1.5),
    b_ub = A_ub x0 + U(0.1, 1), b_eq = A_eq x0, c = A_ub^T(-U(0.1,1)) + A_eq^T N(0,1) + U(0.1,1).
    -> (A_ub, A_eq, A explicit, [(bs, cs structural, cs padded, c0s), ...])"""
    rng = np.random.default_rng([1, nx, m_ub, m_eq])
    A_ub, A_eq = rng.standard_normal((m_ub, nx)), rng.standard_normal((m_eq, nx))
    A = np.zeros((m_ub + m_eq, nx + m_ub))
    A[:m_ub, :nx], A[m_ub:, :nx] = A_ub, A_eq
    A[np.arange(m_ub), nx + np.arange(m_ub)] = 1.0
    sets = []
    for _ in range(nsets):
        bs, cs = [], []
        for _k in range(count):
            x0 = rng.uniform(0.5, 1.5, nx)
            bs.append(np.concatenate([A_ub @ x0 + rng.uniform(0.1, 1.0, m_ub), A_eq @ x0]))
            cs.append(A_ub.T @ (-rng.uniform(0.1, 1.0, m_ub)) + A_eq.T @ rng.standard_normal(m_eq) + rng.uniform(0.1, 1.0, nx))
        sets.append((bs, cs, [np.concatenate([c, np.zeros(m_ub)]) for c in cs], [float(v) for v in rng.uniform(-1.0, 1.0, count)]))
    return A_ub, A_eq, A, sets


def test_structural_slack_forms(built):
    import lp_amd
    m_ub = 70
    A_ub, A_eq, A, ((b0, c0s_, c0p, k0), (b1, c1s, c1p, k1)) = _slack_family()
    o = _opts()
    want_hint = _fresh(lambda cx: cx.upload_lockstep_shared(A, b1, c1p, k1, n_slack=m_ub), o, want_spread=False)
    want_parts = _fresh(lambda cx: cx.upload_lockstep_shared_ub_eq(A_ub, A_eq, b1, c1s, k1), o, want_spread=False)
    _assert_same_members(want_parts, want_hint, "the two references")
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, b0, c0p, k0, n_slack=m_ub)
    assert all(r[0] == 0 for r in ctx.solve_lockstep(o))
    ctx.update_lockstep_vectors(b1, c1p, k1)                      # c in the upload's form: with its slack entries
    _assert_same_members(ctx.solve_lockstep(o), want_hint, "slack hint, after the update")
    ctx.upload_lockstep_shared_ub_eq(A_ub, A_eq, b0, c0s_, k0)
    assert all(r[0] == 0 for r in ctx.solve_lockstep(o))
    ctx.update_lockstep_vectors(b1, c1s, k1)                      # the n structural costs; the slack costs stay 0
    got = ctx.solve_lockstep(o)
    ctx.close()
    _assert_same_members(got, want_parts, "ub / eq blocks, after the update")
    _assert_same_members(got, want_hint, "ub / eq blocks after the update against the slack-hinted batch")


# ---- 6: members with matrices of their own ------------------------------------------------------------------------------------------
def test_own_matrix_batch_keeps_its_factors(built):
    """upload_lockstep: one kept factor per member as before; the update leaves them valid (one launch less afterwards)."""
    import lp_amd
    from lp_amd import synth
    lps = []
    for k in range(4):
        A, b, c, _ = synth.planted_lp(40 + k, 200, 450)
        lps.append((A, b * (1.0 + 3.0 * (k % 3)), c * 10.0 ** (k % 4)))
    As, bs, cs = [p[0] for p in lps], [p[1] for p in lps], [p[2] for p in lps]
    rng = np.random.default_rng(6)
    b2 = [A @ np.where(rng.uniform(size=450) < 0.4, rng.uniform(1.0, 2.0, 450), 0.0) * (1.0 + 3.0 * (k % 3)) for k, A in enumerate(As)]
    c2 = [rng.uniform(0.1, 2.0, 450) * 10.0 ** (k % 4) for k in range(4)]
    o = _opts()
    want0 = _fresh(lambda cx: cx.upload_lockstep(As, bs, cs), o)
    want2 = _fresh(lambda cx: cx.upload_lockstep(As, b2, c2), o)
    ctx = lp_amd.Context(0)
    ctx.set_profiling(1)
    ctx.upload_lockstep(As, bs, cs)
    _assert_same_members(ctx.solve_lockstep(o), want0, "first solve")
    t0 = ctx.phase_times()
    ctx.update_lockstep_vectors(b2, c2)
    _assert_same_members(ctx.solve_lockstep(o), want2, "after the update")
    t2 = ctx.phase_times()
    ctx.close()
    assert t0["iterations"] == max(w[3] for w in want0) and t0["adat_launches"] == t0["iterations"], t0
    assert t2["iterations"] == max(w[3] for w in want2) and t2["adat_launches"] == t2["iterations"] - 1, t2


# ---- 7: partial updates -----------------------------------------------------------------------------------------------------------
def test_partial_updates(built):
    """None leaves what is resident: the result is that of a fresh upload of the old part with the new part.  The constant
    enters fun alone, so c0s=None is checked the same way: against a fresh upload with the constants of the first set."""
    import lp_amd
    seed, m, n, count = 80, 200, 450, 6
    A, ((b0, c0_, k0), (b1, c1, k1)) = _shared_sets(seed, m, n, count)
    o = _opts()
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, b0, c0_, k0)
    ctx.update_lockstep_vectors(bs=None, cs=c1)
    _assert_same_members(ctx.solve_lockstep(o), _fresh(lambda cx: cx.upload_lockstep_shared(A, b0, c1, k0), o), "new c only")
    ctx.update_lockstep_vectors(bs=b1, cs=None, c0s=k1)
    _assert_same_members(ctx.solve_lockstep(o), _shared_ref(seed, m, n, count, 1), "then new b and c0")
    ctx.update_lockstep_vectors(bs=b0, cs=c0_, c0s=None)
    got = ctx.solve_lockstep(o)
    ctx.close()
    _assert_same_members(got, _fresh(lambda cx: cx.upload_lockstep_shared(A, b0, c0_, k1), o), "new b and c, the constants stay")
    want0 = _shared_ref(seed, m, n, count, 0)
    for g, w, ka, kb in zip(got, want0, k1, k0):       # x does not see the constant; fun moves with it
        assert _bits(g[1]) == _bits(w[1]) and g[3] == w[3]
        assert ka != kb and g[2] != w[2]


# ---- 8: device variant ------------------------------------------------------------------------------------------------------------
def test_device_variant_equals_the_host_variant(built):
    import lp_amd
    import torch
    seed, m, n, count = 80, 200, 450, 6
    A, ((b0, c0_, k0), (b1, c1, k1)) = _shared_sets(seed, m, n, count)
    want1 = _shared_ref(seed, m, n, count, 1)
    o = _opts()
    ldb, ldc = m + 5, n + 3
    hb, hc = np.full((count, ldb), np.nan), np.full((count, ldc), np.nan)     # what lies beyond m and n is never read
    hb[:, :m], hc[:, :n] = np.array(b1), np.array(c1)
    dev = torch.device("cuda", 0)
    tb, tc = torch.from_numpy(hb).to(dev), torch.from_numpy(hc).to(dev)
    torch.cuda.synchronize(dev)
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, b0, c0_, k0)
    assert all(r[0] == 0 for r in ctx.solve_lockstep(o))
    ctx.update_lockstep_vectors_device(tb.data_ptr(), ldb, tc.data_ptr(), ldc, k1)
    _assert_same_members(ctx.solve_lockstep(o), want1, "device blocks")
    ctx.update_lockstep_vectors(b0, c0_, k0)
    ctx.update_lockstep_vectors(b1, c1, k1)
    _assert_same_members(ctx.solve_lockstep(o), want1, "host arrays")
    L = lp_amd._capi.lib()
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert L.lpipm_update_lockstep_vectors_device(ctx._h, count, vp(tb), m - 1, vp(tc), ldc, None) == lp_amd._capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_lockstep_vectors_device(ctx._h, count, vp(tb), ldb, vp(tc), n - 1, None) == lp_amd._capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_lockstep_vectors_device(ctx._h, count, None, 0, None, 0, None) == lp_amd._capi.ERR_BAD_ARGUMENT
    _assert_same_members(ctx.solve_lockstep(o), want1, "after the refusals")
    ctx.close()


# ---- 9: bytes ---------------------------------------------------------------------------------------------------------------------
def _kept_bytes(m):
    """include/lpipm.h, lpipm_set_first_factor_cache: 8 mp^2 + 16 sum s_k^2 + 4096 per resident LP; once per shared-matrix batch."""
    mp = -(-m // 128) * 128
    w = 512 if mp <= 2048 else 1024
    return 8 * mp * mp + 16 * sum(min(w, mp - r0) ** 2 for r0 in range(0, mp, w)) + 4096


def _ones_bytes(n):
    """The shared set's vector of ones: one double per padded column (n rounded up to 16), rounded up to 4096 bytes."""
    return -(-(8 * (-(-n // 16) * 16)) // 4096) * 4096


def _resident(upload, on):
    import lp_amd
    ctx = lp_amd.Context(0).set_first_factor_cache(on)
    upload(ctx)
    out = ctx.resident_bytes()
    ctx.close()
    return out


def test_resident_bytes_count_one_set_per_shared_batch(built):
    m, n, count = 128, 300, 18
    rng = np.random.default_rng(0)
    A, b, c = rng.standard_normal((m, n)), rng.standard_normal(m), rng.standard_normal(n)
    shared = lambda cx: cx.upload_lockstep_shared(A, [b] * count, [c] * count)
    own = lambda cx: cx.upload_lockstep([A] * count, [b] * count, [c] * count)
    got = {(name, on): _resident(up, on) for name, up in (("shared", shared), ("own", own)) for on in (True, False)}
    print(f"\n[measure] resident bytes {got}, one kept set {_kept_bytes(m)}, ones {_ones_bytes(n)}")
    # A (mp x npa doubles, a multiple of 4096 bytes) is followed directly by the set; the arenas hold none of it
    assert got["shared", True] - got["shared", False] == _kept_bytes(m) + _ones_bytes(n), got
    assert got["own", True] - got["own", False] == count * _kept_bytes(m), got


# ---- 10: launch counts ------------------------------------------------------------------------------------------------------------
def test_launch_counts_of_a_shared_batch(built):
    """Profiling 1 (one stream): the build's one launch is counted in the first solve; every solve replays the factor."""
    import lp_amd
    seed, m, n, count = 80, 200, 450, 6
    A, (s0, s1) = _shared_sets(seed, m, n, count)
    want0, want1 = _shared_ref(seed, m, n, count, 0), _shared_ref(seed, m, n, count, 1)
    o = _opts()
    ctx = lp_amd.Context(0)
    ctx.set_profiling(1)
    ctx.upload_lockstep_shared(A, *s0)
    seen, wants = [], [want0, want0, want0, want1]
    for k in range(4):
        if k == 3:
            ctx.update_lockstep_vectors(*s1)
        _assert_same_members(ctx.solve_lockstep(o), wants[k], f"solve {k + 1}")
        seen.append(ctx.phase_times())
    ctx.close()
    its = [max(w[3] for w in want) for want in wants]
    assert [t["iterations"] for t in seen] == its, seen
    assert [t["adat_launches"] for t in seen] == [its[0], its[1] - 1, its[2] - 1, its[3] - 1], seen
    assert seen[0]["adat_ms"] > 0.0 and seen[0]["potrf_ms"] > 0.0
    # the later solves factor iterations - 1 times: the build's factorisation is in the first solve's figure alone
    off = _off_context()
    off.set_profiling(1)
    off.upload_lockstep_shared(A, *s0)
    off.solve_lockstep(o)
    t = off.phase_times()
    off.close()
    assert t["adat_launches"] == t["iterations"] == its[0]


# ---- 11: rank-deficient shared A ----------------------------------------------------------------------------------------------------
def test_rank_deficient_shared_matrix_fails_for_every_member(built):
    """A duplicated row: A.A^T has a non-positive pivot, the one kept word goes to every member of every solve."""
    import lp_amd
    from lp_amd import synth, _capi
    m, n, count = 64, 150, 5
    A = synth.planted_lp(4, m, n)[0]
    A[1] = A[0]
    rng = np.random.default_rng(11)
    sets = []
    for _ in range(2):
        bs = [A @ rng.uniform(0.5, 1.5, n) for _k in range(count)]
        sets.append((bs, [rng.uniform(0.1, 2.0, n) for _k in range(count)]))
    o = _opts()
    wants = [_fresh(lambda cx, s=s: cx.upload_lockstep_shared(A, *s), o, want_ok=False, want_spread=False) for s in sets]
    assert all(w[0] == _capi.NUMERICAL_PROBLEM for want in wants for w in want)
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, *sets[0])
    for k in range(2):
        _assert_same_members(ctx.solve_lockstep(o), wants[0], f"solve {k + 1}")
    ctx.update_lockstep_vectors(*sets[1])
    for k in range(2):
        _assert_same_members(ctx.solve_lockstep(o), wants[1], f"after the update, solve {k + 1}")
    ctx.close()


# ---- 12: cache off ------------------------------------------------------------------------------------------------------------------
def test_cache_off_restores_one_factor_per_member_per_solve(built):
    import lp_amd
    seed, m, n, count = 80, 200, 450, 6
    A, (s0, s1) = _shared_sets(seed, m, n, count)
    o = _opts()
    on_bytes = _resident(lambda cx: cx.upload_lockstep_shared(A, *s0), True)
    ctx = lp_amd.Context(0).set_first_factor_cache(False)
    ctx.set_profiling(1)
    ctx.upload_lockstep_shared(A, *s0)
    off_bytes = ctx.resident_bytes()
    _assert_same_members(ctx.solve_lockstep(o), _shared_ref(seed, m, n, count, 0), "first solve")
    ctx.update_lockstep_vectors(*s1)
    _assert_same_members(ctx.solve_lockstep(o), _shared_ref(seed, m, n, count, 1), "after the update")
    t = ctx.phase_times()
    assert t["adat_launches"] == t["iterations"]              # every member forms its own iteration 1
    assert ctx.resident_bytes() == off_bytes == on_bytes - _kept_bytes(m) - _ones_bytes(n)
    ctx.close()


# ---- 13: sweep drivers --------------------------------------------------------------------------------------------------------------
def _same_dicts(got, ref, what):
    assert len(got) == len(ref), what
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g["status"] == r["status"] and g["iterations"] == r["iterations"], (what, i)
        assert _bits(g["x_slack"]) == _bits(r["x_slack"]) and _bits(g["fun"]) == _bits(r["fun"]), (what, i)


def _count_calls(monkeypatch, name):
    import lp_amd
    calls = []
    inner = getattr(lp_amd.Context, name)

    def wrapper(self, *a, **kw):
        calls.append(name)
        return inner(self, *a, **kw)
    monkeypatch.setattr(lp_amd.Context, name, wrapper)
    return calls


def test_sweep_shared_matrix(built, monkeypatch):
    """11 members, max_group 4: 3 chunks of 4, the last one with one repeat of member 10 whose result is dropped."""
    import lp_amd
    from lp_amd import batch
    A, (s0,) = _shared_sets(130, 200, 450, 11, 1)
    o = _opts()
    ref = batch.solve_shared_matrix(A, *s0, opts=o, ctx=_off_context(), max_group=4)
    assert all(r["status"] == 0 for r in ref) and len({r["iterations"] for r in ref}) > 1
    uploads = _count_calls(monkeypatch, "upload_lockstep_shared")
    updates = _count_calls(monkeypatch, "update_lockstep_vectors")
    ctx = lp_amd.Context(0)
    got = batch.sweep_shared_matrix(A, *s0, opts=o, ctx=ctx, max_group=4)
    ctx.close()
    assert len(uploads) == 1 and len(updates) == 2, (uploads, updates)
    _same_dicts(got, ref, "sweep_shared_matrix")


def test_sweep_shared_ub_eq(built, monkeypatch):
    import lp_amd
    from lp_amd import batch
    A_ub, A_eq, _, ((bs, cs, _, k0),) = _slack_family(11, 150, 70, 30, 1)
    o = _opts()
    ref = batch.solve_shared_ub_eq(A_ub, A_eq, bs, cs, k0, opts=o, ctx=_off_context(), max_group=4)
    assert all(r["status"] == 0 for r in ref)
    uploads = _count_calls(monkeypatch, "upload_lockstep_shared_ub_eq")
    updates = _count_calls(monkeypatch, "update_lockstep_vectors")
    ctx = lp_amd.Context(0)
    got = batch.sweep_shared_ub_eq(A_ub, A_eq, bs, cs, k0, opts=o, ctx=ctx, max_group=4)
    ctx.close()
    assert len(uploads) == 1 and len(updates) == 2, (uploads, updates)
    _same_dicts(got, ref, "sweep_shared_ub_eq")


# ---- 14: refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_resident_batch_as_it_was(built):
    import lp_amd
    from lp_amd import _capi
    L = _capi.lib()
    seed, m, n, count = 80, 200, 450, 6
    A, ((b0, c0_, k0), (b1, c1, k1)) = _shared_sets(seed, m, n, count)
    dp = C.POINTER(C.c_double)
    arr = lambda lst: (dp * len(lst))(*[a.ctypes.data_as(dp) for a in lst])
    ctx = lp_amd.Context(0)
    assert L.lpipm_update_lockstep_vectors(ctx._h, count, arr(b1), arr(c1), None) == _capi.ERR_NO_PROBLEM
    ctx.upload_lockstep_shared(A, b0, c0_, k0)
    assert L.lpipm_update_lockstep_vectors(ctx._h, count - 1, arr(b1[:-1]), arr(c1[:-1]), None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_lockstep_vectors(ctx._h, count + 1, arr(b1 + b1[:1]), arr(c1 + c1[:1]), None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_lockstep_vectors(ctx._h, count, None, None, (C.c_double * count)(*k1)) == _capi.ERR_BAD_ARGUMENT
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        ctx.update_lockstep_vectors(b1[:-1], c1[:-1])
    _assert_same_members(ctx.solve_lockstep(_opts()), _shared_ref(seed, m, n, count, 0), "after the refusals")
    rng = np.random.default_rng(1)
    x0 = rng.uniform(0.1, 1.0, 40)
    A_ub = rng.uniform(0.0, 1.0, (30, 40)); A_eq = rng.standard_normal((10, 40))
    prob = lp_amd.Problem.target(rng.standard_normal(40)).ub(A_ub, A_ub @ x0 + 0.5).eq(A_eq, A_eq @ x0).build()
    ctx.upload(prob)                                                                       # lpipm_upload_ub_eq
    bb, cc = np.zeros(40), np.zeros(70)
    assert L.lpipm_update_lockstep_vectors(ctx._h, 1, arr([bb]), arr([cc]), None) == _capi.ERR_UNSUPPORTED
    ctx.close()
