"""Checkers for the passes over A (the GEMVs) and for one IPM iteration against plain references (test infrastructure).

GEMVs: a componentwise bound against an extended-precision reference.  Whatever the order in which a kernel sums the k
products of an output, with or without fused multiply-adds, the float64 result y satisfies

    |y - A w| <= gamma_k (|A| |w|),   gamma_k = k u / (1 - k u),   u = 2^-53

(Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5).  check_gemv asserts |got - ref| <= 2 k u (|A| |w|)
elementwise: no measured number enters it, and it is far stricter than a normwise bound on the rows whose magnitude is
small.  The reference is summed in np.longdouble (64-bit significand on x86-64), so its own error is 2^-11 of the bound.
Dropping one product from a sum moves that output by |a_ij w_j|, which is about 1 / (2 k u) times the bound.

One iteration: iteration_envelope runs oracle.iteration on the LP as given and on the same LP with its columns permuted
(A[:, P], c[P], x[P], z[P]), un-permutes the second result, and keeps the spread between the two.  check_iteration then
holds each quantity of the device's iteration to max(fixed * scale, K * spread) around the first run: the oracle
envelope of tests/golden/c4_members.npz, one permutation wide.
"""
import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64
_LD = np.longdouble
_ROWS = 512                         # row band of the blocked extended-precision products (bounds the temporaries)

VEC_KEYS = ("x", "y", "z", "d_x", "d_y", "d_z")
SCALAR_KEYS = ("tau", "kappa", "d_tau", "d_kappa", "alpha")


def _extended():
    assert np.finfo(_LD).nmant >= 63, "the GEMV references need an extended-precision np.longdouble (x86-64)"


def gemv_n_ref(A, W):
    """A w for each row w of W (nrhs x n, or one vector of n), in np.longdouble.
    -> (ref, mag): ref[q] = A w_q and mag[q] = |A| |w_q|, both nrhs x m (extended precision)."""
    _extended()
    W = np.atleast_2d(np.asarray(W, dtype=np.float64)).astype(_LD)
    m = A.shape[0]
    ref = np.empty((W.shape[0], m), dtype=_LD)
    mag = np.empty((W.shape[0], m), dtype=_LD)
    for i0 in range(0, m, _ROWS):
        B = A[i0:i0 + _ROWS].astype(_LD)
        ref[:, i0:i0 + _ROWS] = W @ B.T
        mag[:, i0:i0 + _ROWS] = np.abs(W) @ np.abs(B).T
    return ref, mag


def gemv_t_ref(A, V):
    """A^T v for each row v of V (nrhs x m, or one vector of m), in np.longdouble.
    -> (ref, mag): ref[q] = A^T v_q and mag[q] = |A^T| |v_q|, both nrhs x n (extended precision)."""
    _extended()
    V = np.atleast_2d(np.asarray(V, dtype=np.float64)).astype(_LD)
    m, n = A.shape
    ref = np.zeros((V.shape[0], n), dtype=_LD)
    mag = np.zeros((V.shape[0], n), dtype=_LD)
    for i0 in range(0, m, _ROWS):
        B = A[i0:i0 + _ROWS].astype(_LD)
        Vb = V[:, i0:i0 + _ROWS]
        ref += Vb @ B
        mag += np.abs(Vb) @ np.abs(B)
    return ref, mag


def gemv_ratio(got, ref, mag, k):
    """max over the outputs of |got - ref| / (2 k u mag).  An output whose magnitude is 0 must be exact (ratio inf if not)."""
    got = np.atleast_2d(np.asarray(got, dtype=np.float64))
    err = np.abs(got.astype(_LD) - ref)
    bound = 2 * k * _LD(U) * mag
    if not np.all(np.isfinite(got)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    return float(r.max()) if r.size else 0.0


def check_gemv(got, ref, mag, k, what=""):
    """Assert |got - ref| <= 2 k u mag elementwise (k: the number of products in each output); returns the largest ratio
    of the error to the bound."""
    r = gemv_ratio(got, ref, mag, k)
    assert r <= 1.0, f"{what}: |got - ref| / (2 k u |A||w|) = {r:.3g} > 1 (k = {k})"
    return r


# ---------------------------------------------------------------------------------------------------------------------
def iteration_envelope(A, b, c, x, y, z, tau, kappa, ip=False, seed=0):
    """oracle.iteration on (A, b, c) from the iterate, and on the LP with its columns permuted by a random P (seeded).
    -> (ref, spread): ref is the first run; spread[k] = max |ref[k] - run2[k]| (run2 un-permuted) for every quantity."""
    from oracle import capi as oracle
    n = A.shape[1]
    P = np.random.default_rng(seed).permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[P] = np.arange(n)
    ref = oracle.iteration(A, b, c, x, y, z, tau, kappa, ip=ip)
    alt = oracle.iteration(np.ascontiguousarray(A[:, P]), b, c[P], x[P], y, z[P], tau, kappa, ip=ip)
    assert ref["status"] == 0 and alt["status"] == 0, (ref["status"], alt["status"])
    for k in ("x", "z", "d_x", "d_z"):
        alt[k] = alt[k][inv]
    spread = {k: float(np.abs(ref[k] - alt[k]).max()) for k in VEC_KEYS}
    spread.update({k: abs(ref[k] - alt[k]) for k in SCALAR_KEYS})
    return ref, spread


def iteration_ratios(dev, ref, spread, fixed=1e-8, K=4.0):
    """For each quantity: max |dev - ref| / max(fixed * max(1, max|ref|), K * spread).  alpha is held to `fixed` absolute."""
    out = {}
    for k in VEC_KEYS + SCALAR_KEYS:
        d, r = np.asarray(dev[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        err = float(np.abs(d - r).max()) if np.all(np.isfinite(d)) else float("inf")
        scale = 1.0 if k == "alpha" else max(1.0, float(np.abs(r).max()))
        out[k] = err / max(fixed * scale, K * spread[k])
    return out


def check_iteration(dev, ref, spread, fixed=1e-8, K=4.0):
    """Assert every ratio of iteration_ratios <= 1; returns the ratios."""
    assert dev.get("info", 0) == 0 and ref["status"] == 0
    r = iteration_ratios(dev, ref, spread, fixed, K)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"outside max({fixed:g} scale, {K:g} spread): {bad}"
    return r


def spread_multiples(dev, ref, spread, fixed=1e-8):
    """max |dev - ref| / spread for each quantity whose error exceeds the fixed bound (0 for the others; inf where the two
    oracle runs agree exactly): what K has to cover."""
    out = {}
    for k in VEC_KEYS + SCALAR_KEYS:
        r = np.asarray(ref[k], dtype=np.float64)
        err = float(np.abs(np.asarray(dev[k], dtype=np.float64) - r).max())
        scale = 1.0 if k == "alpha" else max(1.0, float(np.abs(r).max()))
        if err <= fixed * scale:
            out[k] = 0.0
        else:
            out[k] = err / spread[k] if spread[k] > 0 else float("inf")
    return out
