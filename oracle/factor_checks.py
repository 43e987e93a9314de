"""Checkers for a Cholesky factor and a solve against plain float64 / extended-precision references (test infrastructure).

Every checker returns a dimensionless number -- the measured error divided by the unit its bound is stated in -- so that
a test asserts `value <= c` with one constant c for every size.

  factor_residual_c(L, M)    max_{i>=j} |fl(L L^T) - M|_ij / (s_i s_j)  /  ((m+1) u),   s_i = ||L[i,:]||_2
  probe_residual_c(L, M, X)  max_i |L (L^T x) - M x|_i / (s_i (s.|x|))  /  ((m+1) u),   max over the columns x of X
  forward_error(v, vt)       ||v - vt||_inf / ||vt||_inf
  solve_residual(M, v, r)    ||M v - r||_inf / (||M||_inf ||v||_inf + ||r||_inf)

For a backward-stable Cholesky (LAPACK's) |L L^T - M| <= c (m+1) u |L| |L^T| (Higham, Accuracy and Stability of Numerical
Algorithms, Thm 10.3), and by Cauchy-Schwarz (|L| |L^T|)_ij <= s_i s_j: factor_residual_c <= c with a small c.  The extra
m u covers the float64 product L L^T the check forms itself.  Scaling by s_i s_j instead of max|M| resolves rows whose
scale is far below the largest one, which a norm-wise check cannot see.  The probe variant bounds the same error through
O(m^2) products: sum_j |dM_ij| |x_j| <= c (m+1) u s_i (s.|x|).
"""
import numpy as np
import scipy.linalg as sla

U = 2.0 ** -53          # unit roundoff of float64
_ROWS = 1024            # row band of the blocked products (bounds the temporaries at large m)

# Bounds the GPU factor and solve are held to on the well-conditioned family (well_conditioned below, kappa <= 60;
# tests/test_gpu_factor_at_scale.py), in the units of the checkers.  Set from an MI355X run at m = 1100 .. 16384 with
# 5-9x headroom over the largest value measured (in brackets).
FACTOR_C = 0.1          # factor_residual_c and probe_residual_c                [0.0138, at m = 1100]
FACTOR_L = 1.0          # max|L - L_lapack| / (kappa u max|L|)                  [0.178]
SOLVE_RES_C = 2e-3      # solve_residual / ((m+1) u)                            [2.3e-4]
SOLVE_FWD_C = 5e-3      # forward_error / (kappa (m+1) u)                       [7.5e-4]


def row_norms(L):
    """s_i = ||L[i, :]||_2 of the lower triangle of L."""
    s = np.empty(L.shape[0])
    for i0 in range(0, L.shape[0], _ROWS):
        B = np.tril(L[i0:i0 + _ROWS], i0)
        s[i0:i0 + _ROWS] = np.sqrt(np.einsum("ij,ij->i", B, B))
    return s


def factor_residual_c(L, M):
    """max over the lower triangle of |fl(L L^T) - M|_ij / (s_i s_j), in units of (m+1) u.
    Only the lower triangles of L and M are read."""
    m = L.shape[0]
    Lt = np.tril(L)
    s = row_norms(Lt)
    worst = 0.0
    for i0 in range(0, m, _ROWS):
        i1 = min(m, i0 + _ROWS)
        R = np.abs(Lt[i0:i1, :i1] @ Lt[:i1, :i1].T - M[i0:i1, :i1])
        R /= np.outer(s[i0:i1], s[:i1])
        worst = max(worst, float(np.tril(R, i0).max()))
    return worst / ((m + 1) * U)


def probe_columns(m, rng, nrand=4):
    """Probe vectors (columns of an m x p matrix): `nrand` standard normal ones, and unit vectors e_k at the first and
    last column of every 128-block boundary, outer panel (512) and super-block (1024) edge, and the last column m-1."""
    ks = {0, m - 1}
    for edge in (128, 512, 1024):
        for b in range(edge, m, edge):
            ks.update((b - 1, b))
    ks = sorted(k for k in ks if 0 <= k < m)
    # at large m the 128-block boundaries alone are hundreds of probes: keep every outer-panel edge and at most 64 others
    if len(ks) > 96:
        big = [k for k in ks if k % 512 in (0, 511) or k == m - 1]
        rest = [k for k in ks if k not in big]
        ks = sorted(set(big) | set(rest[:: max(1, len(rest) // 64)]))
    X = np.zeros((m, nrand + len(ks)))
    X[:, :nrand] = rng.standard_normal((m, nrand))
    X[ks, nrand + np.arange(len(ks))] = 1.0
    return X


def probe_residual_c(L, M, X):
    """max_i |L (L^T x) - M x|_i / (s_i (s.|x|)) over the columns x of X, in units of (m+1) u.
    M is the symmetric matrix (both triangles); only the lower triangle of L is read."""
    m = L.shape[0]
    Lt = np.tril(L)
    s = row_norms(Lt)
    R = np.abs(Lt @ (Lt.T @ X) - M @ X)
    R /= np.outer(s, s @ np.abs(X))
    return float(R.max()) / ((m + 1) * U)


def solve_residual(M, v, r):
    """||M v - r||_inf / (||M||_inf ||v||_inf + ||r||_inf): the normwise backward error of v (M symmetric, both triangles)."""
    return float(np.abs(M @ v - r).max() / (np.abs(M).sum(axis=1).max() * np.abs(v).max() + np.abs(r).max()))


def forward_error(v, vt):
    """||v - vt||_inf / ||vt||_inf (vt may be np.longdouble)."""
    vt = np.asarray(vt)
    return float(np.abs(np.asarray(v, dtype=vt.dtype) - vt).max() / np.abs(vt).max())


def refined_solution(M, r, cf=None, steps=8):
    """The solution of M v = r (r: one right-hand side, or an m x k block of them) to about extended precision: LAPACK's
    Cholesky solve (scipy cho_factor / cho_solve, or the lower factor `cf` = (L, True) given), refined `steps` times with
    residuals formed in np.longdouble.  -> (v as np.longdouble, cf)."""
    if cf is None:
        cf = sla.cho_factor(M, lower=True)
    cf = (np.asfortranarray(cf[0]), cf[1])        # LAPACK's layout: no copy of the factor inside every cho_solve
    LD = np.longdouble
    Ml = M.astype(LD)
    rl = np.asarray(r).astype(LD)
    v = sla.cho_solve(cf, r).astype(LD)
    for _ in range(steps):
        res = (rl - Ml @ v).astype(np.float64)
        v = v + sla.cho_solve(cf, res).astype(LD)
    return v, cf


def well_conditioned(m, seed, k=64, kappa=60.0):
    """M = D + U U^T (U m x k, D positive diagonal), dense with every 128 x 128 tile nonzero and distinct, and a cheap
    upper bound on its 2-norm condition number: (max D + ||U||_2^2) / min D.  -> (M, kappa_bound)."""
    rng = np.random.default_rng([seed, m, k])
    d = rng.uniform(1.0, 2.0, m)
    U_ = rng.standard_normal((m, k))
    U_ *= np.sqrt((kappa - 2.0) / np.linalg.eigvalsh(U_.T @ U_).max())     # ||U||_2^2 = kappa - 2
    M = U_ @ U_.T
    M[np.diag_indices(m)] += d
    return M, float((d.max() + (kappa - 2.0)) / d.min())


def adat_lower(A, d):
    """(A diag(d) A^T) with only its lower triangle formed (row bands; the upper triangle is zero)."""
    m = A.shape[0]
    M = np.zeros((m, m))
    for i0 in range(0, m, _ROWS):
        i1 = min(m, i0 + _ROWS)
        M[i0:i1, :i1] = (A[i0:i1] * d) @ A[:i1].T
    return np.tril(M)
