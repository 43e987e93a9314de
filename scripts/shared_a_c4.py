#!/usr/bin/env python3
"""C4 shard (32 x 1024x2048) of scenarios that share ONE constraint matrix (synth.planted_scenarios), solved as
  (a) copies : lpipm_upload_lockstep with 32 copies of A (one per member arena), and
  (b) shared : lpipm_upload_lockstep_shared (A resident once, every pass over it serving the whole batch).
Prints LP/s of each (resident inputs, median of --steps timed solves), the per-lockstep-iteration phase split of one extra
profiled solve (lpipm_set_profiling(1): one stream, every phase bracketed by events), resident bytes, and a member-by-member
bit comparison of (a) and (b)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=32)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import lp_amd
    from lp_amd import synth
    A, bs, cs, xstars = synth.planted_scenarios(0, args.m, args.n, args.count)
    o = lp_amd.InteriorPoint.default().opts()
    out, results = {}, {}
    for name in ("copies", "shared"):
        ctx = lp_amd.Context(0)
        if name == "copies":
            ctx.upload_lockstep([A] * args.count, bs, cs)
        else:
            ctx.upload_lockstep_shared(A, bs, cs)
        for _ in range(args.warmup):
            ctx.solve_lockstep(o)
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            res = ctx.solve_lockstep(o)
            times.append(time.perf_counter() - t0)
        results[name] = res
        ctx.set_profiling(1)
        ctx.solve_lockstep(o)
        pt = ctx.phase_times()
        ctx.set_profiling(0)
        it = max(pt["iterations"], 1)
        out[name] = dict(lp_per_s=round(args.count / float(np.median(times)), 1),
                         solve_ms_median=round(1e3 * float(np.median(times)), 3),
                         per_iteration_ms={k: round(pt[k + "_ms"] / it, 4) for k in ("adat", "potrf", "trsv", "gemv", "vec", "total")},
                         lockstep_iterations=int(pt["iterations"]), gemv_passes=int(pt["gemv_passes"]),
                         resident_bytes=ctx.resident_bytes())
        ctx.close()
    a, b = results["copies"], results["shared"]
    same = [a[i][0] == b[i][0] and a[i][3] == b[i][3] and np.array_equal(a[i][1], b[i][1]) for i in range(args.count)]
    err = max(float(np.abs(b[i][1] - xstars[i]).max()) for i in range(args.count) if b[i][1] is not None)
    out["members_bit_identical"] = f"{sum(same)}/{args.count}"
    out["max_abs_x_minus_planted"] = err
    out["resident_bytes_saved"] = out["copies"]["resident_bytes"] - out["shared"]["resident_bytes"]
    out["lp_per_s_ratio"] = round(out["shared"]["lp_per_s"] / out["copies"]["lp_per_s"], 4)
    print(json.dumps(out, indent=1))
    return 0 if all(same) else 1


if __name__ == "__main__":
    sys.exit(main())
