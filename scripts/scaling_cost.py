#!/usr/bin/env python3
"""Measurements behind profiles/scaling.md (power-of-two equilibration at upload).

  scaling_cost.py upload [--rounds R]   upload-to-ready (host clock around the synchronous upload call) with 0, 4 and 8
                                        passes, the three settings alternated inside every round, at 4096x8192 (one LP) and
                                        32 x 1024x2048 (a lockstep batch whose members own their matrices); medians and the
                                        spread per setting, and the iterations of one solve per setting
  scaling_cost.py trace                 upload 4096x8192 and the 32 x 1024x2048 batch once with 8 passes: the program of the
                                        kernel trace, whose k_scale_* rows are the device time of the new launches
                                        (rocprofv3 --kernel-trace --stats -- python scripts/scaling_cost.py trace)

Prints one JSON line.  Fails without a GPU: there is nothing to fall back to."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"4096x8192": (1, 4096, 8192), "32x1024x2048": (32, 1024, 2048)}
PASSES = (0, 4, 8)


def expected_ms(count, m, n, passes):
    """Arithmetic only: `passes` reads of A, then one read and one write of it, at the 6 TB/s the microarchitecture guide
    gives as achievable."""
    return (passes + 2) * count * m * n * 8 / 6e12 * 1e3 if passes else 0.0


def members(count, m, n):
    from lp_amd import synth
    return [synth.planted_lp(s, m, n)[:3] for s in range(count)]


def upload(ctx, lps):
    if len(lps) == 1:
        ctx.upload_arrays(*lps[0])
    else:
        ctx.upload_lockstep([p[0] for p in lps], [p[1] for p in lps], [p[2] for p in lps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("upload", "trace"))
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import lp_amd
    out = {"mode": args.mode}
    opts = lp_amd.InteriorPoint.default().opts()
    for name, (count, m, n) in SHAPES.items():
        lps = members(count, m, n)
        ctxs = {p: lp_amd.Context(0).set_scaling(p) for p in (PASSES if args.mode == "upload" else (8,))}
        for ctx in ctxs.values():
            upload(ctx, lps)                                   # warm-up: allocations, code objects
        if args.mode == "trace":
            upload(ctxs[8], lps)
            out[name] = {"uploads_with_8_passes": 2}
        else:
            ms = {p: [] for p in PASSES}
            for _ in range(args.rounds):
                for p in PASSES:                               # alternated: a drift of the box hits all three alike
                    t0 = time.perf_counter()
                    upload(ctxs[p], lps)
                    ms[p].append((time.perf_counter() - t0) * 1e3)
            its = {}
            for p in PASSES:
                res = ctxs[p].solve_raw(opts) if count == 1 else ctxs[p].solve_lockstep(opts)
                its[p] = res[3] if count == 1 else max(r[3] for r in res)
            out[name] = {str(p): {"upload_ms_median": round(statistics.median(ms[p]), 3), "upload_ms_min": round(min(ms[p]), 3),
                                  "upload_ms_max": round(max(ms[p]), 3), "expected_scaling_ms": round(expected_ms(count, m, n, p), 3),
                                  "iterations": int(its[p]), "resident_bytes": ctxs[p].resident_bytes()} for p in PASSES}
        for ctx in ctxs.values():
            ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
