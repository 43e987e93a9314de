#!/usr/bin/env python
"""Measurements behind profiles/first_factor_cache.md (the first iteration's factor kept per upload).

  first_factor_cache.py first [--off]   first and second solve after a fresh upload, median of 5 uploads, at 4096x8192 and
                                        512x1024 (--off: lpipm_set_first_factor_cache(ctx, 0), the behaviour before)
  first_factor_cache.py twice           upload 4096x8192 and solve twice: the program of the kernel trace
                                        (rocprofv3 --kernel-trace --stats -- python scripts/first_factor_cache.py twice)
One JSON line on stdout."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lp_amd                      # noqa: E402
from lp_amd import synth           # noqa: E402


def fresh(on):
    ctx = lp_amd.Context(0)
    if hasattr(ctx, "set_first_factor_cache"):
        ctx.set_first_factor_cache(on)
    return ctx


def first(on):
    out = {"first_factor_cache": on}
    o = lp_amd.InteriorPoint.default().opts()
    for (m, n) in ((4096, 8192), (512, 1024)):
        A, b, c, _ = synth.planted_lp(0, m, n)
        warm = fresh(on); warm.upload_arrays(A, b, c); warm.solve_raw(o); warm.close()     # code objects loaded, clocks up
        t_first, t_second = [], []
        for _ in range(5):
            ctx = fresh(on)
            ctx.upload_arrays(A, b, c)
            t0 = time.perf_counter()
            rc, _, _, it, _ = ctx.solve_raw(o)
            t1 = time.perf_counter()
            ctx.solve_raw(o)
            t2 = time.perf_counter()
            ctx.close()
            assert rc == 0
            t_first.append((t1 - t0) * 1e3); t_second.append((t2 - t1) * 1e3)
        out[f"{m}x{n}"] = {"iterations": it, "first_ms": t_first, "first_median_ms": statistics.median(t_first),
                           "second_ms": t_second, "second_median_ms": statistics.median(t_second)}
    print(json.dumps(out))


def twice():
    A, b, c, _ = synth.planted_lp(0, 4096, 8192)
    ctx = fresh(True)
    ctx.upload_arrays(A, b, c)
    o = lp_amd.InteriorPoint.default().opts()
    res = [ctx.solve_raw(o) for _ in range(2)]
    ctx.close()
    print(json.dumps({"status": [r[0] for r in res], "iterations": [r[3] for r in res], "fun": [r[2] for r in res]}))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "twice":
        twice()
    else:
        first("--off" not in sys.argv)
