"""CPU check of the coupled sweep's rounding (profiles/solve_coupled.md): the plain super-block sweep and the coupled one
(H_k = Inv_k^T L[k+1,k]^T, G_k = Inv_k L[k,k-1], kernels_trsv.hip) transcribed in NumPy on LAPACK's factor, on the matrices of
tests/test_gpu_factor_at_scale.py.  Prints the figures that file asserts, for each sweep and each choice of G / H.

    python scripts/coupled_sweep_accuracy.py            # needs no GPU
"""
import os
import sys

import numpy as np
import scipy.linalg as sla

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import factor_checks as fc   # noqa: E402
from lp_amd import synth                 # noqa: E402

U = fc.U


def blocks(m, w):
    return [(r, min(m, r + w)) for r in range(0, m, w)]


def inverses(L, sb):
    return [sla.solve_triangular(L[a:b, a:b], np.eye(b - a), lower=True) for a, b in sb]


def sweep_plain(L, sb, inv, r):
    r = r.copy()
    y = np.zeros_like(r)
    for k, (a, b) in enumerate(sb):
        y[a:b] = inv[k] @ r[a:b]
        r[b:] -= L[b:, a:b] @ y[a:b]
    v = np.zeros_like(r)
    for k in range(len(sb) - 1, -1, -1):
        a, b = sb[k]
        v[a:b] = inv[k].T @ (y[a:b] - L[b:, a:b].T @ v[b:])
    return v


def sweep_coupled(L, sb, inv, r, use_g=True, use_h=True):
    n = len(sb)
    H = [inv[k].T @ L[sb[k + 1][0]:sb[k + 1][1], sb[k][0]:sb[k][1]].T if k < n - 1 else None for k in range(n)]
    G = [inv[k] @ L[sb[k][0]:sb[k][1], sb[k - 1][0]:sb[k - 1][1]] if 1 <= k <= n - 2 else None for k in range(n)]
    t = r.copy()
    y = np.zeros_like(r)
    if not use_g:
        for k, (a, b) in enumerate(sb):
            y[a:b] = inv[k] @ t[a:b]
            t[b:] -= L[b:, a:b] @ y[a:b]
    else:
        for k, (a, b) in enumerate(sb):
            if k == 0:
                y[a:b] = inv[k] @ t[a:b]
                continue
            pa, pb = sb[k - 1]
            if k == n - 1:
                t[a:b] -= L[a:b, pa:pb] @ y[pa:pb]
                y[a:b] = inv[k] @ t[a:b]
                continue
            y[a:b] = inv[k] @ t[a:b] - G[k] @ y[pa:pb]
            t[b:] -= L[b:, pa:pb] @ y[pa:pb]
    s = y.copy()
    v = np.zeros_like(r)
    for k in range(n - 1, -1, -1):
        a, b = sb[k]
        if k == n - 1:
            v[a:b] = inv[k].T @ s[a:b]
            continue
        na, nb = sb[k + 1]
        if use_h:
            v[a:b] = inv[k].T @ s[a:b] - H[k] @ v[na:nb]
        else:
            v[a:b] = inv[k].T @ (s[a:b] - L[na:nb, a:b].T @ v[na:nb])
        s[:a] -= L[na:nb, :a].T @ v[na:nb]
    return v


def report(label, M, r, w, kappa=None):
    m = M.shape[0]
    cf = sla.cho_factor(M, lower=True)
    L = np.tril(cf[0])
    sb = blocks(m, w)
    inv = inverses(L, sb)
    vt = fc.refined_solution(M, r, cf=(L, True))[0]
    f_lap = fc.forward_error(sla.cho_solve((L, True), r), vt)
    for name, v in (("plain", sweep_plain(L, sb, inv, r)), ("coupled G+H", sweep_coupled(L, sb, inv, r)),
                    ("coupled H only", sweep_coupled(L, sb, inv, r, use_g=False)),
                    ("coupled G only", sweep_coupled(L, sb, inv, r, use_h=False))):
        res = fc.solve_residual(M, v, r) / ((m + 1) * U)
        fwd = fc.forward_error(v, vt)
        extra = f"forward c {fwd / (kappa * (m + 1) * U):.3g}" if kappa else f"forward {fwd:.3g} / lapack {f_lap:.3g} = {fwd / f_lap:.3g}"
        print(f"[measure] {label} w={w} nsb={len(sb)} {name:15s}: residual c {res:.3g}, {extra}")


def main():
    for m, w in ((2500, 512), (4096, 1024)):
        M, kappa = fc.well_conditioned(m, 5)
        R = np.random.default_rng(m + 1).standard_normal((2, m))
        report(f"well m={m} rhs 1", M, R[0], w, kappa)
        report(f"well m={m} rhs 1e8", M, R[0] * 1e8, w, kappa)
    for m, dkind, w in ((2500, "log", 512), (4096, "log", 1024), (4096, "basis", 1024)):
        A, b, c, xs = synth.planted_lp(9, m, 2 * m)
        rng = np.random.default_rng([m, len(dkind)])
        if dkind == "log":
            d = 10.0 ** rng.uniform(-8, 8, 2 * m)
        else:
            d = np.where(xs > 0, 10.0 ** rng.uniform(2, 8, 2 * m), 10.0 ** rng.uniform(-8, -2, 2 * m))
        Ml = fc.adat_lower(A, d)
        M = np.tril(Ml) + np.tril(Ml, -1).T
        report(f"late m={m} {dkind}", M, b + A @ (d * c), w)


if __name__ == "__main__":
    main()
