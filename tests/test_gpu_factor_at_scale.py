"""The factorisation, the solve and A.D.A^T at the sizes where the library switches to its large-size schedules, against
plain references (oracle/factor_checks.py).  Which branch each shape reaches follows from the host-side dispatch rules:

  m      mp / nb      factorisation and solve (super_for, trailing_update_columns, launch_potrf, factor_plan_create)
  1100   1152 / 9     512-wide super-blocks, the last one a single block; serial schedule
  2049   2176 / 17    1024-wide super-blocks (mp > 2048), the last one a single block
  2500   2560 / 20    1024-wide super-blocks and a partial 4-block one
  4096   4096 / 32    look-ahead on (nb >= 32); 64-edge and 32x32 trailing updates; 4 full super-blocks
  7000   7040 / 55    128-edge trailing updates (remT (remT+1)/2 >= 1024: the serial updates behind panels 0 and 1, the
                      look-ahead "rest" behind panel 0); last outer panel 3 blocks; last super-block 7 blocks (merges
                      [0,4)+[4,7), [4,6)+[6,7)); 40 padded rows
  16384  16384 / 128  the C5 factor: probe checks only

  A.D.A^T, single LP, default knobs (plan_adat, launch_adat): the round-2 kernel (gemm_nt_streamk_w8_kernel) and its
  fix-up (gemm_nt_fixup_kernel) where the units kernel is not taken --
  (768, 2048)    21 tiles x 8 chunks < 256 units: round-2, every tile stream-K, KT = 128 <= 256
  (1025, 1100)   45 tiles x 5 chunks < 256 units: round-2, every tile stream-K, KT = 69
  (7000, 17000)  units slabs 1540 x 22 x 128 KiB > 4 GiB: round-2, KT = 1063, 16-k-tile stream-K units, 4 fix-up tiles
  (1024, 8192)   LPIPM_ADAT_UNITS=0: round-2, KT = 512, every tile stream-K
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import factor_checks as fc

pytestmark = pytest.mark.gpu

U = fc.U


@functools.lru_cache(maxsize=1)
def _wc(m):
    """The well-conditioned matrix of size m, its condition bound and numpy's factor of it (one size cached at a time)."""
    M, kappa = fc.well_conditioned(m, 5)
    Lnp = np.linalg.cholesky(M) if m <= 8192 else None
    return M, kappa, Lnp


def _truth(M, Lnp, r):
    return fc.refined_solution(M, r, cf=(Lnp, True))[0]


# ---------------------------------------------------------------------------------------------------------------------
# well-conditioned family: fixed bounds
@pytest.mark.parametrize("m", [1100, 2049, 2500, 4096, 7000])
def test_factor_and_solve_well_conditioned(ctx, m):
    """M = D + U U^T with kappa(M) <= 60.  Factor: scaled componentwise residual and probe residual <= FACTOR_C (m+1) u,
    and |L - L_numpy| <= FACTOR_L kappa u max|L|.  Solve, nrhs 1 and 2 (the second with right-hand sides of scale 1e8 and
    1e-8, so that mixed-up slabs show): backward error <= SOLVE_RES_C (m+1) u and forward error against an
    extended-precision refined solution <= SOLVE_FWD_C kappa (m+1) u, every right-hand side on its own scale."""
    M, kappa, Lnp = _wc(m)
    L, info, _ = ctx.k_potrf(M)
    assert info == 0
    L = np.tril(L)
    cf = fc.factor_residual_c(L, M)
    cp = fc.probe_residual_c(L, M, fc.probe_columns(m, np.random.default_rng(m)))
    dl = float(np.abs(L - Lnp).max() / np.abs(Lnp).max()) / (kappa * U)
    print(f"\n[measure] well m={m}: factor c {cf:.3g}, probe c {cp:.3g}, |L - L_np| / (kappa u max|L|) {dl:.3g}")
    assert cf <= fc.FACTOR_C, cf
    assert cp <= fc.FACTOR_C, cp
    assert dl <= fc.FACTOR_L, dl
    rng = np.random.default_rng(m + 1)
    R = rng.standard_normal((2, m))
    R2 = R * np.array([[1e8], [1e-8]])
    truth = _truth(M, Lnp, np.stack([R[0], R2[0], R2[1]], axis=1))
    for RR, T in ((R[:1], truth[:, :1]), (R2, truth[:, 1:])):
        V, _ = ctx.k_chol_solve(m, RR)
        for q in range(RR.shape[0]):
            res = fc.solve_residual(M, V[q], RR[q]) / ((m + 1) * U)
            fwd = fc.forward_error(V[q], T[:, q]) / (kappa * (m + 1) * U)
            print(f"[measure] well m={m} nrhs={RR.shape[0]} q={q}: residual c {res:.3g}, forward c {fwd:.3g}")
            assert res <= fc.SOLVE_RES_C, res
            assert fwd <= fc.SOLVE_FWD_C, fwd


# ---------------------------------------------------------------------------------------------------------------------
def test_factor_and_solve_bits_at_7000(ctx, built, monkeypatch):
    """m = 7000: three factorisations and solves give the same bits, and the default schedule (look-ahead: the "rest"
    update behind panel 0 on 128-edge tiles, then 64-edge ones) gives the bits of LPIPM_LOOKAHEAD=0 (128-edge tiles behind
    panels 0 and 1 on the chain): every element is the same k-ordered sum whatever the tile edge and the stream."""
    import lp_amd
    m = 7000
    M, _, _ = _wc(m)
    R = np.random.default_rng(3).standard_normal((2, m))
    L0, info, _ = ctx.k_potrf(M)
    V0, _ = ctx.k_chol_solve(m, R)
    assert info == 0
    L0 = np.tril(L0)
    for _ in range(2):
        L, info, _ = ctx.k_potrf(M)
        V, _ = ctx.k_chol_solve(m, R)
        assert info == 0 and np.array_equal(np.tril(L), L0) and np.array_equal(V, V0)
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_LOOKAHEAD", "0")
    serial = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_LOOKAHEAD")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    L1, info, _ = serial.k_potrf(M)
    V1, _ = serial.k_chol_solve(m, R)
    serial.close()
    assert info == 0 and np.array_equal(np.tril(L1), L0) and np.array_equal(V1, V0)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k", [(7000, 0), (7000, 127), (7000, 128), (7000, 511), (7000, 512), (7000, 3000),
                                 (7000, 6999), (1100, 0), (1100, 1099)])
def test_potrf_reports_the_first_nonpositive_pivot(ctx, m, k):
    """include/lpipm.h: info = k+1 for the FIRST non-positive pivot.  M[k,k] -= 2 Lref[k,k]^2 leaves every pivot before k
    as it was and makes pivot k exactly -Lref[k,k]^2.  k = 3000 is a column the look-ahead updates on its side stream;
    k = 6999 the last real row (partial last outer panel and super-block)."""
    M, _, Lnp = _wc(m)
    Mk = M.copy()
    Mk[k, k] -= 2.0 * Lnp[k, k] ** 2
    _, info, _ = ctx.k_potrf(Mk)
    assert info == k + 1, info


# ---------------------------------------------------------------------------------------------------------------------
def test_factor_and_solve_c5_probes(ctx):
    """m = 16384 (C5, 128 blocks, 16 super-blocks): probe residual <= FACTOR_C (m+1) u, and the solve's backward error
    <= SOLVE_RES_C (m+1) u.  No O(m^3) reference at this size."""
    m = 16384
    M, kappa, _ = _wc(m)
    L, info, _ = ctx.k_potrf(M)
    assert info == 0
    cp = fc.probe_residual_c(L, M, fc.probe_columns(m, np.random.default_rng(m)))
    del L
    R = np.random.default_rng(m + 1).standard_normal((2, m)) * np.array([[1e8], [1e-8]])
    V, _ = ctx.k_chol_solve(m, R)
    res = [fc.solve_residual(M, V[q], R[q]) / ((m + 1) * U) for q in range(2)]
    print(f"\n[measure] well m={m}: probe c {cp:.3g}, residual c {res[0]:.3g} {res[1]:.3g}")
    _wc.cache_clear()
    assert cp <= fc.FACTOR_C, cp
    assert max(res) <= fc.SOLVE_RES_C, res


# ---------------------------------------------------------------------------------------------------------------------
# late-IPM normal equations: against LAPACK on the same matrix
def _late_ipm_check(ctx, M, r, label):
    m = M.shape[0]
    L, info, _ = ctx.k_potrf(M)
    assert info == 0
    cfac = sla.cho_factor(M, lower=True)
    c_gpu, c_lap = fc.factor_residual_c(L, M), fc.factor_residual_c(cfac[0], M)
    V, _ = ctx.k_chol_solve(m, r)
    vt = fc.refined_solution(M, r, cf=cfac)[0]
    f_gpu, f_lap = fc.forward_error(V[0], vt), fc.forward_error(sla.cho_solve(cfac, r), vt)
    print(f"\n[measure] late {label}: factor c gpu {c_gpu:.3g} lapack {c_lap:.3g} ratio {c_gpu / c_lap:.3g}; "
          f"forward gpu {f_gpu:.3g} lapack {f_lap:.3g} ratio {f_gpu / f_lap:.3g}")
    assert c_gpu <= LATE_FACTOR_RATIO * c_lap + LATE_FACTOR_FLOOR, (c_gpu, c_lap)
    assert f_gpu <= LATE_FWD_RATIO * f_lap + LATE_FWD_FLOOR * m * U, (f_gpu, f_lap)


# GPU / LAPACK on the same matrix, measured on an MI355X (factor_residual_c ratio; forward error ratio):
#   m = 1100 log 1.35, 1.10 | 2049 log 1.85, 1.97 | 2500 log 1.78, 1.73 | 4096 log 1.72, 0.95
#   m = 1100 basis 1.34, 0.39 | 4096 basis 2.29, 0.83 | C4 last iterate 2.00, 0.44
# (absolute: factor c 0.003 .. 0.018; forward errors 5e-8 .. 7e-7, LAPACK's 5e-8 .. 1.6e-6)
LATE_FACTOR_RATIO, LATE_FACTOR_FLOOR = 4.0, 0.005      # floor in factor_residual_c units
LATE_FWD_RATIO, LATE_FWD_FLOOR = 4.0, 1.0              # floor in units of m u


def _symmetric(M):
    return np.tril(M) + np.tril(M, -1).T


@pytest.mark.parametrize("m,dkind", [(1100, "log"), (2049, "log"), (2500, "log"), (4096, "log"), (1100, "basis"),
                                     (4096, "basis")])
def test_late_ipm_normal_equations_match_lapack(ctx, m, dkind):
    """M = A diag(d) A^T, A = synth.planted_lp(m, 2m), d = 10^U(-8, 8) ("log") or 10^U(2, 8) on the planted basis and
    10^U(-8, -2) off it ("basis"); r = b + A (d c), the first right-hand side of a sym_solve.  The GPU's scaled factor
    residual and its solve's forward error (against an extended-precision refined solution) must be within a fixed
    factor of LAPACK's (scipy cho_factor / cho_solve) on the same matrix, above a small absolute floor.  Measured: the
    GPU factor's scaled residual is 1.3 - 2.3x LAPACK's, its forward error 0.4 - 2.0x LAPACK's (table above
    LATE_FACTOR_RATIO): the unrefined explicit-inverse solve with 1024-wide super-blocks is as accurate as a substitution."""
    from lp_amd import synth
    A, b, c, xs = synth.planted_lp(9, m, 2 * m)
    rng = np.random.default_rng([m, len(dkind)])
    if dkind == "log":
        d = 10.0 ** rng.uniform(-8, 8, 2 * m)
    else:
        d = np.where(xs > 0, 10.0 ** rng.uniform(2, 8, 2 * m), 10.0 ** rng.uniform(-8, -2, 2 * m))
    M = _symmetric(fc.adat_lower(A, d))
    _late_ipm_check(ctx, M, b + A @ (d * c), f"m={m} {dkind}")


def test_late_ipm_c4_last_iterate_matches_lapack(ctx):
    """The C4 shape (1024 x 2048, planted seed 73) at the start of the numpy oracle's last iteration, traced as
    scripts/solve_accuracy.py does: d = x/z there spans about 1e-9 .. 1e9 and cond(M) is about 3e12.  Measured: factor
    residual 2.0x LAPACK's, forward error 7.1e-7 against LAPACK's 1.6e-6."""
    from lp_amd import synth
    from oracle import oracle_np
    A, b, c, _ = synth.planted_lp(73, 1024, 2048)
    tr = []
    oracle_np.solve(A, b, c, trace=tr)
    x, _, z, _, _ = tr[-1]
    d = x / z
    M = _symmetric(A @ (d[:, None] * A.T))
    _late_ipm_check(ctx, M, b + A @ (d * c), "C4 last iterate")


# ---------------------------------------------------------------------------------------------------------------------
def _adat_check(cx, A, d):
    """k_adat against numpy on the lower triangle, the tolerance of test_gpu_kernels.test_adat_matches_oracle."""
    Mg, _ = cx.k_adat(d)
    ref = fc.adat_lower(A, d)
    il = np.tril_indices(A.shape[0])
    err = np.abs(Mg[il] - ref[il]).max()
    print(f"\n[measure] adat {A.shape}: err / (sqrt(n) max|M|) {err / (np.sqrt(A.shape[1]) * np.abs(ref).max()):.3g}")
    assert err <= 1e-13 * np.sqrt(A.shape[1]) * np.abs(ref).max(), err
    return Mg, il


@pytest.mark.parametrize("m,n", [(768, 2048), (1025, 1100)])
def test_adat_round2_default_small(ctx, built, monkeypatch, m, n):
    """The round-2 kernel with its fix-up at KT <= 256 (the default for these shapes): against numpy, and bit-identical to
    the units kernel (LPIPM_ADAT_UNITS=2) -- the head of kernels_adat.hip: M's bits do not depend on the decomposition."""
    import lp_amd
    rng = np.random.default_rng(m * n)
    A = rng.standard_normal((m, n))
    d = np.exp(rng.uniform(-6, 6, n))
    ctx.upload_arrays(A, np.zeros(m), np.zeros(n))
    M0, il = _adat_check(ctx, A, d)
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_ADAT_UNITS", "2")
    cx = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_ADAT_UNITS")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    cx.upload_arrays(A, np.zeros(m), np.zeros(n))
    M1, _ = cx.k_adat(d)
    cx.close()
    assert np.array_equal(M1[il], M0[il])


def test_adat_round2_default_large(ctx):
    """(7000, 17000): the units kernel's slabs would exceed 4 GiB, so the default is the round-2 kernel with KT = 1063,
    16-k-tile stream-K units and a fix-up launch.  Against numpy, and three launches give the same bits."""
    m, n = 7000, 17000
    rng = np.random.default_rng(17)
    A = rng.standard_normal((m, n))
    d = np.exp(rng.uniform(-6, 6, n))
    ctx.upload_arrays(A, np.zeros(m), np.zeros(n))
    M0, il = _adat_check(ctx, A, d)
    for _ in range(2):
        M1, _ = ctx.k_adat(d)
        assert np.array_equal(M1[il], M0[il])


def test_adat_round2_forced_long_contraction(built, monkeypatch):
    """(1024, 8192) with LPIPM_ADAT_UNITS=0: the round-2 kernel's KT > 256 regime (16-k-tile stream-K units, every tile
    through the fix-up) at a small m.  Against numpy, and reproducible."""
    import lp_amd
    m, n = 1024, 8192
    rng = np.random.default_rng(8192)
    A = rng.standard_normal((m, n))
    d = np.exp(rng.uniform(-6, 6, n))
    monkeypatch.setenv("LPIPM_EXPERIMENTAL", "1")
    monkeypatch.setenv("LPIPM_ADAT_UNITS", "0")
    cx = lp_amd.Context(0)
    monkeypatch.delenv("LPIPM_ADAT_UNITS")
    monkeypatch.delenv("LPIPM_EXPERIMENTAL")
    cx.upload_arrays(A, np.zeros(m), np.zeros(n))
    M0, il = _adat_check(cx, A, d)
    M1, _ = cx.k_adat(d)
    cx.close()
    assert np.array_equal(M1[il], M0[il])
