#!/usr/bin/env python
"""Measurements behind profiles/tall_form.md (the tall inequality form).

  tall_form.py compare    ms per iteration and the phase split (lpipm_set_profiling(1)) of lpipm_upload_ub_tall and of
                          lpipm_upload_ub_eq on the same planted LP, at (m_ub, nx) = (4096, 256) and (16384, 512); the
                          end-to-end time per iteration is taken with profiling off (host clock around solves that end in a
                          device synchronise), median of 5 after one warm-up solve
  tall_form.py big        the tall path alone at (131072, 512): resident bytes, time per iteration, the launch that builds K
                          (adat_ms / adat_launches) and its share of the fp64 MFMA peak, useful flop = nx (nx + 1) m per launch
                          (the lower triangle of K, 2 flop per multiply-add)
One JSON line on stdout."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lp_amd                      # noqa: E402

PEAK_FP64_MFMA_TFLOPS = 78.6       # bench.py's roofline denominator


def planted(seed, m, nx):
    """tests/test_gpu_tall_form.py's generator: a planted nondegenerate vertex of min c.x, X x <= b, x >= 0."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    k = nx // 2
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:k]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, k)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    return X, b, -X.T @ lam + mu, xs


def measure(prob, tall, xs, repeats=5):
    o = lp_amd.InteriorPoint.default().opts()
    ctx = lp_amd.Context(0)
    ctx.upload(prob, tall=tall)
    out = {"resident_bytes": ctx.resident_bytes()}
    rc, x, fun, it, _ = ctx.solve_raw(o)                      # warm-up: code objects loaded, clocks up (and the kept first factor)
    out.update(status=rc, iterations=it, err_x=float(np.abs(x[:xs.shape[0]] - xs).max()))
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ctx.solve_raw(o)
        times.append((time.perf_counter() - t0) * 1e3)
    out["solve_ms_median"] = statistics.median(times)
    out["solve_ms_min_max"] = [min(times), max(times)]
    out["ms_per_iteration"] = out["solve_ms_median"] / it
    ctx.set_profiling(1)
    ctx.solve_raw(o)
    out["phases"] = ctx.phase_times()
    ctx.set_profiling(0)
    ctx.close()
    return out


def compare():
    res = {}
    for (m, nx) in ((4096, 256), (16384, 512)):
        X, b, c, xs = planted(0, m, nx)
        prob = lp_amd.Problem.target(c).ub(X, b).build()
        res[f"{m}x{nx}"] = {"tall": measure(prob, True, xs), "ub_eq": measure(prob, False, xs)}
    return res


def big():
    m, nx = 131072, 512
    X, b, c, xs = planted(0, m, nx)
    r = measure(lp_amd.Problem.target(c).ub(X, b).build(), True, xs, repeats=3)
    ph = r["phases"]
    launch_ms = ph["adat_ms"] / max(1, ph["adat_launches"])
    r["k_build_ms_per_launch"] = launch_ms
    r["k_build_tflops"] = nx * (nx + 1) * m / (launch_ms * 1e-3) / 1e12
    r["k_build_frac_of_fp64_mfma_peak"] = r["k_build_tflops"] / PEAK_FP64_MFMA_TFLOPS
    return {f"{m}x{nx}": {"tall": r}}


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "compare"
    print(json.dumps({"mode": mode, **(compare() if mode == "compare" else big())}))
