"""The vector stage of an iteration and the passes over A at the sizes where they run their multi-workgroup code, against
plain references (oracle/vector_checks.py).  Which branch each shape reaches follows from the host-side rules:
mp = m rounded up to 128, npa = stored (structural) columns rounded up to 16, nblk = min(512, ceil(max(m, n) / 256))
(upload_impl), the fused single-workgroup vector kernels only while nblk <= 4 (vec_fused, FUSED_USE_NBLK), A.x chunk
slabs ax_chunks = gemv_dual_chunks(npa), row splits nsplit = mp / 128, and gemv_dual's chunk width CW = 1024 from
npa >= 4096, else 256 (launch_gemv_dual).

  m x n (slack)      nblk  vector stage   elems/thread  ax_chunks  nsplit  CW    what it adds
  1025 x 1100          5   plain          1             5          9       256   just past the fused limit; m > 1024
  1100 x 2300          9   plain          1             9          9       256   m not a multiple of 128, n of 256
  1024 x 2048          8   plain          1             8          8       256   the C4 member shape
  2048 x 4096         16   plain          1             4          16      1024
  4096 x 8192         32   plain          1             8          32      1024  the C3 headline
  300 x 140000       512   plain          2             137        3       1024  nblk capped: a thread's second element
  64 x 270000        512   plain          3             264        1       1024  a thread's third element
  1500 x 4300 (1000)  17   plain          1             11         12      256   ub / eq problem, 1000 slack columns
  300 x 140300 (300) 512   plain          2             137        3       1024  slack columns past the stored 140000
  GEMVs:
  1100 x 4097         17   -              -             5          9       1024  last chunk 16 columns wide
  16384 x 2048        64   -              -             8          128     256   128 row splits
  1100|4096 x 4080     -   -              -             16         9|32    256   the widest CW = 256 launch
  1100|4096 x 4095     -   -              -             4          9|32    1024  (npa = 4096: CW = 1024, like 4096)
  1100|4096 x 9000     -   -              -             9          9|32    1024  last chunk 816 columns wide
  1100 x 4797 (700)   19   -              -             5          9       1024  slack: 700 identity rows of 1100

Bounds.  GEMVs: componentwise, |got - ref| <= 2 k u |A| |w| against an extended-precision reference (no tuning).  One
iteration: every quantity within max(1e-8 max(1, max|ref|), K spread) of oracle.iteration, where spread is the
difference between the oracle's run and its run on the column-permuted LP; K = 4 for random interior iterates (where the
fixed 1e-8 governs) and K = LATE_K for the last iterates of a solve, where d = x / z spans 1e-9 .. 1e9 and the oracle does
not agree with itself to 1e-8.
"""
import functools

import numpy as np
import pytest

from oracle import vector_checks as vc

pytestmark = pytest.mark.gpu

# max |dev - ref| / spread over the quantities that the fixed 1e-8 does not cover, on the last three iterates of the planted
# 1024 x 2048 LP (seed 0), measured on an MI355X in two runs: at most 25.3 (alpha of the last iterate; 8.0 for the vectors).
# The iterates come from numpy's BLAS, so they differ slightly between machines.  Committed with 5x headroom.
LATE_K = 128.0
SECOND = 131072                  # 512 workgroups x 256 threads: index SECOND + t is thread t's second element


def _iterate(rng, m, n, spread):
    x = np.exp(rng.uniform(-spread, spread, n)); z = np.exp(rng.uniform(-spread, spread, n))
    return x, rng.standard_normal(m), z, float(np.exp(rng.uniform(-1, 1))), float(np.exp(rng.uniform(-1, 1)))


@functools.lru_cache(maxsize=2)
def _planted(seed, m, n):
    from lp_amd import synth
    return synth.planted_lp(seed, m, n)[:3]


def _with_slack(A, c, ns):
    """[A | S] with S = [I_ns; 0]: the slack-form matrix of ns inequality rows (linear_program.rs:145-156)."""
    m = A.shape[0]
    S = np.zeros((m, ns))
    S[np.arange(ns), np.arange(ns)] = 1.0
    return np.hstack([A, S]), np.concatenate([c, np.zeros(ns)])


def _blocker(ref, x, z, tau, kappa):
    """(what limits the step, its index) per get_step_size (feasible_point.rs:53-72); ('none', -1) at a full step."""
    dx, dz = ref["d_x"], ref["d_z"]
    rx = np.where(dx < 0, x / -np.where(dx < 0, dx, -1.0), np.inf)
    rz = np.where(dz < 0, z / -np.where(dz < 0, dz, -1.0), np.inf)
    cand = {"x": (rx.min(), int(rx.argmin())), "z": (rz.min(), int(rz.argmin())),
            "tau": (tau / -ref["d_tau"] if ref["d_tau"] < 0 else np.inf, -1),
            "kappa": (kappa / -ref["d_kappa"] if ref["d_kappa"] < 0 else np.inf, -1)}
    k = min(cand, key=lambda q: cand[q][0])
    return (k, cand[k][1]) if cand[k][0] < 1.0 else ("none", -1)


def _one(ctx, A, b, c, x, y, z, tau, kappa, ip, seed, K=4.0, what=""):
    import lp_amd as lp
    ref, spread = vc.iteration_envelope(A, b, c, x, y, z, tau, kappa, ip=ip, seed=seed)
    dev = ctx.k_iteration(lp.InteriorPoint.default().opts(), x, y, z, tau, kappa, ip=ip)
    r = vc.check_iteration(dev, ref, spread, K=K)
    print(f"\n[measure] {what} ip={ip}: worst ratio {max(r.values()):.3g} ({max(r, key=r.get)})")
    if ip:                                              # ip arm: alpha = 1 and the clamp at 1 (feasible_point.rs:96-105)
        assert dev["alpha"] == 1.0 and dev["x"].min() >= 1.0 and dev["z"].min() >= 1.0
        assert dev["tau"] >= 1.0 and dev["kappa"] >= 1.0
    return dev, ref, spread


# ---------------------------------------------------------------------------------------------------------------------
# one iteration from random interior iterates, the plain multi-workgroup vector kernels
@pytest.mark.parametrize("m,n,seed,ip", [(m, n, s, ip) for (m, n, s) in
                                         [(1025, 1100, 1), (1100, 2300, 2), (1024, 2048, 3), (2048, 4096, 4),
                                          (300, 140000, 5), (64, 270000, 6)] for ip in (False, True)]
                         + [(4096, 8192, 7, False)])
def test_one_iteration_at_scale(ctx, m, n, seed, ip):
    A, b, c = _planted(seed, m, n)
    ctx.upload_arrays(A, b, c)
    x, y, z, tau, kappa = _iterate(np.random.default_rng(100 * seed + int(ip)), m, n, 1.5)
    dev, ref, _ = _one(ctx, A, b, c, x, y, z, tau, kappa, ip, seed, what=f"{m}x{n}")
    if not ip:
        assert (ref["d_x"] < 0).any() and (ref["d_x"] > 0).any()
        assert ref["alpha"] < 0.99995                     # the ratio test decided the step


def test_one_iteration_ub_eq_problem_with_slack_columns(ctx):
    """Context.upload(problem) of a ub / eq problem: 1000 of the 4300 columns are slack columns, never stored, added by
    slack_n_kernel / slack_t_kernel inside the residual pass and every GEMV of the iteration."""
    import lp_amd as lp
    A0, b0, c0 = _planted(8, 1500, 3300)
    prob = lp.Problem.target(c0).ub(A0[:1000], b0[:1000]).eq(A0[1000:], b0[1000:]).build()
    A, b, c = prob.A(), prob.b(), prob.c()
    assert A.shape == (1500, 4300) and prob.n_slack() == 1000
    ctx.upload(prob)
    for ip in (False, True):
        x, y, z, tau, kappa = _iterate(np.random.default_rng(80 + int(ip)), 1500, 4300, 1.5)
        _one(ctx, A, b, c, x, y, z, tau, kappa, ip, 8, what="ub/eq 1500x4300 (1000 slack)")


def test_one_iteration_with_slack_columns_past_the_second_element(ctx):
    """upload_arrays(..., n_slack=300) at 300 x 140300: the slack columns sit at indices 140000 .. 140299, in the second
    element of threads 8928 .. 9227."""
    A0, b, c0 = _planted(9, 300, 140000)
    A, c = _with_slack(A0, c0, 300)
    ctx.upload_arrays(A, b, c, n_slack=300)
    for ip in (False, True):
        x, y, z, tau, kappa = _iterate(np.random.default_rng(90 + int(ip)), 300, 140300, 1.5)
        _one(ctx, A, b, c, x, y, z, tau, kappa, ip, 9, what="300x140300 (300 slack)")


# ---------------------------------------------------------------------------------------------------------------------
# the ratio test at n > 131072: the blocking element in a thread's second element
def _ratio_case(target):
    """(A, b, c, x, y, z, tau, kappa) of a 300 x 140000 LP whose step is limited by `target`.  x and z: the planted LP's
    column that limits the step (found by the oracle) is swapped with column n - 1 (thread 8927's second element)."""
    from oracle import capi as oracle
    m, n = 300, 140000
    A, b, c = _planted(21, m, n)
    x, y, z = np.full(n, 10.0), np.zeros(m), np.full(n, 10.0)
    sc, tau, kappa = {"x": (1.0, 1e-4, 1.0), "z": (-1.0, 1e-4, 1.0), "tau": (-1.0, 1e-4, 1e-4)}[target]
    c = sc * c
    if target in ("x", "z"):
        r0 = oracle.iteration(A, b, c, x, y, z, tau, kappa)
        k, j = _blocker(r0, x, z, tau, kappa)
        assert k == target, (k, j)
        P = np.arange(n)
        P[[j, n - 1]] = P[[n - 1, j]]
        A, c = np.ascontiguousarray(A[:, P]), c[P]
    return A, b, c, x, y, z, tau, kappa


@pytest.mark.parametrize("target", ["x", "z", "tau"])
def test_ratio_test_blocked_past_the_first_element(ctx, target):
    A, b, c, x, y, z, tau, kappa = _ratio_case(target)
    n = A.shape[1]
    ctx.upload_arrays(A, b, c)
    dev, ref, _ = _one(ctx, A, b, c, x, y, z, tau, kappa, False, 21, what=f"blocked by {target}")
    assert n - 1 >= SECOND
    want = (target, n - 1) if target in ("x", "z") else (target, -1)
    assert _blocker(ref, x, z, tau, kappa) == want
    assert _blocker(dev, x, z, tau, kappa) == want
    assert dev["alpha"] < 0.5


# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _late_trace():
    from oracle import oracle_np
    A, b, c = _planted(0, 1024, 2048)
    tr = []
    res = oracle_np.solve(A, b, c, trace=tr)
    assert res.status == 0
    return A, b, c, tr


@pytest.mark.parametrize("back", [3, 2, 1])
def test_late_iterates_within_the_oracle_envelope(ctx, back):
    """The iterates at the start of the last three iterations of the oracle's solve of the planted 1024 x 2048 LP (seed 0):
    d = x / z spans 4e-6 .. 1e4, 2e-7 .. 3e5 and 8e-10 .. 5e8, and the two oracle orderings differ by up to 2e-7 in y.
    Every quantity must lie within LATE_K times that spread (or 1e-8 relative)."""
    A, b, c, tr = _late_trace()
    x, y, z, tau, kappa = tr[-back]
    ctx.upload_arrays(A, b, c)
    import lp_amd as lp
    ref, spread = vc.iteration_envelope(A, b, c, x, y, z, tau, kappa, seed=back)
    dev = ctx.k_iteration(lp.InteriorPoint.default().opts(), x, y, z, tau, kappa)
    mult = vc.spread_multiples(dev, ref, spread)
    d = x / z
    print(f"\n[measure] late -{back}: d in [{d.min():.2g}, {d.max():.2g}], |dev - ref| / spread: "
          + ", ".join(f"{k} {v:.3g}" for k, v in mult.items()))
    r = vc.check_iteration(dev, ref, spread, K=LATE_K)
    print(f"[measure] late -{back}: worst ratio {max(r.values()):.3g} ({max(r, key=r.get)})")


# ---------------------------------------------------------------------------------------------------------------------
# bit properties of the plain path
def test_iteration_bits_repeat_at_nblk_512(ctx):
    A, b, c = _planted(5, 300, 140000)
    ctx.upload_arrays(A, b, c)
    import lp_amd as lp
    o = lp.InteriorPoint.default().opts()
    x, y, z, tau, kappa = _iterate(np.random.default_rng(55), 300, 140000, 1.5)
    runs = [ctx.k_iteration(o, x, y, z, tau, kappa) for _ in range(3)]
    for r in runs[1:]:
        for k, v in runs[0].items():
            assert np.array_equal(np.asarray(v), np.asarray(r[k])), k


@pytest.mark.parametrize("m,n", [(1100, 2300), (300, 140000)])
def test_folded_scalars_equal_the_separate_scalar_kernels(built, m, n):
    """Single GPU: the one-wave scalar steps are folded into their consumers (every workgroup folds the partials itself).
    World 1 through the column-split entry points runs them as their own kernels (k_scalar_dtau, k_scalar_alpha, k_fold):
    the solve must have the same bits."""
    import lp_amd
    A, b, c = _planted(10, m, n)
    opts = lp_amd.InteriorPoint.default().opts()
    cx = lp_amd.Context(0)
    cx.upload_arrays(A, b, c)
    rc0, x0, f0, it0, log0 = cx.solve_raw(opts, want_log=True)
    cx.set_collective(0, 1, None)
    cx.upload_column_block(A, b, c, n)
    rc1, x1, f1, it1, log1 = cx.solve_raw(opts, want_log=True)
    cx.close()
    print(f"\n[measure] {m}x{n}: {it0} iterations")
    assert (rc0, it0) == (rc1, it1) and rc0 == 0
    assert np.array_equal(x0, x1) and f0 == f1 and log0 == log1


def test_lockstep_members_equal_single_solves_at_nblk_512(built):
    """Three members of 64 x 140000 in one lockstep batch: each member's reduction slots are its own (512 partials per
    slot), so each must come out bit-identical to its single solve."""
    import lp_amd
    probs = [_planted(s, 64, 140000) for s in (30, 31, 32)]
    opts = lp_amd.InteriorPoint.default().opts()
    cx = lp_amd.Context(0)
    singles = []
    for A, b, c in probs:
        cx.upload_arrays(A, b, c)
        singles.append(cx.solve_raw(opts))
    cx.upload_lockstep([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs])
    lock = cx.solve_lockstep(opts)
    cx.close()
    for (rc, x, f, it, _), (st, xl, fl, itl) in zip(singles, lock):
        assert rc == st == 0 and it == itl
        assert np.array_equal(x, xl) and f == fl


# ---------------------------------------------------------------------------------------------------------------------
# GEMVs against the extended-precision reference, componentwise
def _scaled(rng, m, n):
    """A standard normal matrix with row and column scales 2^U(-8, 8): a normwise bound cannot see its small rows."""
    return rng.standard_normal((m, n)) * np.exp2(rng.uniform(-8, 8, m))[:, None] * np.exp2(rng.uniform(-8, 8, n))[None, :]


def _check_n_t(ctx, A, rng, order=(1, 2), what=""):
    m, n = A.shape
    W = rng.standard_normal((2, n)) * np.exp2(rng.uniform(-6, 6, n))
    V = rng.standard_normal((2, m)) * np.exp2(rng.uniform(-6, 6, m))
    (yn, mn), (yt, mt) = vc.gemv_n_ref(A, W), vc.gemv_t_ref(A, V)
    worst = [0.0, 0.0]
    for nrhs in order:
        Y, _ = ctx.k_gemv_n(W[:nrhs])
        U, _ = ctx.k_gemv_t(V[:nrhs])
        worst[0] = max(worst[0], vc.check_gemv(Y, yn[:nrhs], mn[:nrhs], n, f"{what} gemv_n nrhs={nrhs}"))
        worst[1] = max(worst[1], vc.check_gemv(U, yt[:nrhs], mt[:nrhs], m, f"{what} gemv_t nrhs={nrhs}"))
    print(f"\n[measure] {what} {m}x{n}: gemv_n ratio {worst[0]:.3g}, gemv_t ratio {worst[1]:.3g}")


@pytest.mark.parametrize("m,n", [(1100, 4097), (4096, 8192), (16384, 2048), (300, 140000)])
def test_gemv_n_t_componentwise(ctx, m, n):
    rng = np.random.default_rng(m + n)
    A = _scaled(rng, m, n)
    ctx.upload_arrays(A, np.zeros(m), np.zeros(n))
    _check_n_t(ctx, A, rng, what="dense")


def _check_dual(ctx, A, rng, what=""):
    m, n = A.shape
    w = rng.standard_normal(n) * np.exp2(rng.uniform(-6, 6, n))
    v = rng.standard_normal(m) * np.exp2(rng.uniform(-6, 6, m))
    (yn, mn), (yt, mt) = vc.gemv_n_ref(A, w), vc.gemv_t_ref(A, v)
    Aw, ATv, _ = ctx.k_gemv_dual(w, v)
    rn = vc.check_gemv(Aw, yn, mn, n, f"{what} dual A.w")
    rt = vc.check_gemv(ATv, yt, mt, m, f"{what} dual A^T.v")
    print(f"\n[measure] {what} dual {m}x{n}: A.w ratio {rn:.3g}, A^T.v ratio {rt:.3g}")


@pytest.mark.parametrize("m", [1100, 4096])
@pytest.mark.parametrize("n", [4080, 4095, 4096, 4097, 9000])
def test_gemv_dual_componentwise(ctx, m, n):
    rng = np.random.default_rng(7 * m + n)
    A = _scaled(rng, m, n)
    ctx.upload_arrays(A, np.zeros(m), np.zeros(n))
    _check_dual(ctx, A, rng, what="dense")


@pytest.mark.parametrize("m,nx,ns", [(1100, 4097, 700), (1500, 2800, 1500), (4096, 8192, 4096)])
def test_gemvs_with_slack_columns_componentwise(ctx, m, nx, ns):
    """The slack columns' identity block through slack_n_kernel / slack_t_kernel, in gemv_n, gemv_t (2 vectors, then 1)
    and gemv_dual."""
    rng = np.random.default_rng(m + nx + ns)
    A, _ = _with_slack(_scaled(rng, m, nx), np.zeros(nx), ns)
    ctx.upload_arrays(A, np.zeros(m), np.zeros(nx + ns), n_slack=ns)
    _check_n_t(ctx, A, rng, order=(2, 1), what=f"slack {ns}")
    _check_dual(ctx, A, rng, what=f"slack {ns}")


def test_gemv_t_one_vector_after_two_with_slack_columns(ctx):
    """slack_t_kernel writes an explicit 0 into every row split but the first: the slab buffer of the 2-vector layout
    ([split][q]) overlaps the 1-vector one ([split]), so a split it left alone would keep a value of the 2-vector call."""
    m, nx, ns = 1100, 3000, 900
    rng = np.random.default_rng(4)
    A, _ = _with_slack(_scaled(rng, m, nx), np.zeros(nx), ns)
    ctx.upload_arrays(A, np.zeros(m), np.zeros(nx + ns), n_slack=ns)
    V2 = rng.standard_normal((2, m)) * 1e3
    v1 = rng.standard_normal((1, m))
    ctx.k_gemv_t(V2)
    U, _ = ctx.k_gemv_t(v1)
    yt, mt = vc.gemv_t_ref(A, v1)
    vc.check_gemv(U, yt, mt, m, "gemv_t nrhs=1 after nrhs=2")
    assert np.array_equal(U[0, nx:], v1[0, :ns])
