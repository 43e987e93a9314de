#!/usr/bin/env python3
"""32 inequality-form LPs of (nx, m_ub, m_eq) = (1024, 1024, 0) -- BASELINE config 4's member shape, 1024 x 2048 in slack
form, half of it identity -- from one scenario family (tests/test_gpu_slack_batches.py has the generator), one context per
variant:
  (a) shared dense : the explicit slack-form matrix through lpipm_upload_lockstep_shared (what was possible before),
  (b) shared ub_eq : lpipm_upload_lockstep_shared_ub_eq (the slack block structural),
  (c) copies dense : the explicit matrix, one copy per member, through lpipm_upload_lockstep,
  (d) copies slack : the same through lpipm_upload_lockstep_slack.
All four are resident at once; the timed solves ALTERNATE a, b, c, d, a, ... (median of --steps each), and (a) is timed a
second time in every round ("a2") to show the spread of one variant against itself.  Then, per variant, one extra solve with
lpipm_set_profiling(1) (one stream, every phase bracketed by events): per-phase ms per lockstep iteration, resident bytes,
iteration counts.  --trace V solves only variant V, --steps times after one warm-up: the body of a kernel-trace run."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def family(nx, m_ub, count, seed=1):
    rng = np.random.default_rng([seed, nx, m_ub, 0])
    A_ub = rng.standard_normal((m_ub, nx))
    bs, cs = [], []
    for _ in range(count):
        x0 = rng.uniform(0.5, 1.5, nx)
        bs.append(A_ub @ x0 + rng.uniform(0.1, 1.0, m_ub))
        cs.append(A_ub.T @ (-rng.uniform(0.1, 1.0, m_ub)) + rng.uniform(0.1, 1.0, nx))
    return A_ub, bs, cs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=32)
    ap.add_argument("--nx", type=int, default=1024)
    ap.add_argument("--m-ub", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", choices=["a", "b", "c", "d"], default=None)
    args = ap.parse_args()
    import lp_amd
    K, nx, m_ub = args.count, args.nx, args.m_ub
    A_ub, bs, cs = family(nx, m_ub, K)
    A = np.hstack([A_ub, np.eye(m_ub)])
    csp = [np.concatenate([c, np.zeros(m_ub)]) for c in cs]
    o = lp_amd.InteriorPoint.default().opts()
    uploads = {
        "a": ("shared dense", lambda c: c.upload_lockstep_shared(A, bs, csp)),
        "b": ("shared ub_eq", lambda c: c.upload_lockstep_shared_ub_eq(A_ub, None, bs, cs)),
        "c": ("copies dense", lambda c: c.upload_lockstep([A] * K, bs, csp)),
        "d": ("copies slack", lambda c: c.upload_lockstep([A] * K, bs, csp, n_slack=m_ub)),
    }
    if args.trace:
        ctx = lp_amd.Context(0)
        uploads[args.trace][1](ctx)
        for _ in range(args.warmup + args.steps):
            res = ctx.solve_lockstep(o)
        print(json.dumps(dict(variant=uploads[args.trace][0], iterations=[r[3] for r in res])))
        return 0
    ctxs = {k: lp_amd.Context(0) for k in uploads}
    for k, (_, up) in uploads.items():
        up(ctxs[k])
        for _ in range(args.warmup):
            ctxs[k].solve_lockstep(o)
    order = ["a", "b", "c", "d", "a2"]
    times = {k: [] for k in order}
    results = {}
    for _ in range(args.steps):
        for k in order:
            ctx = ctxs[k[0]]
            t0 = time.perf_counter()
            results[k[0]] = ctx.solve_lockstep(o)
            times[k].append(time.perf_counter() - t0)
    out = {}
    for k in order:
        name = uploads[k[0]][0] + (" (again)" if k == "a2" else "")
        out[name] = dict(lp_per_s=round(K / float(np.median(times[k])), 1), solve_ms_median=round(1e3 * float(np.median(times[k])), 3),
                         solve_ms_all=[round(1e3 * t, 3) for t in times[k]])
    for k, (name, _) in uploads.items():
        ctx = ctxs[k]
        ctx.set_profiling(1)
        ctx.solve_lockstep(o)
        pt = ctx.phase_times()
        ctx.set_profiling(0)
        it = max(pt["iterations"], 1)
        out[name].update(per_iteration_ms={p: round(pt[p + "_ms"] / it, 4) for p in ("adat", "potrf", "trsv", "gemv", "vec", "total")},
                         lockstep_iterations=int(pt["iterations"]), resident_bytes=ctx.resident_bytes(),
                         statuses=sorted({r[0] for r in results[k]}), member_iterations=[r[3] for r in results[k]])
    same = lambda p, q: sum(a[0] == b[0] and a[3] == b[3] and np.array_equal(a[1], b[1]) for a, b in zip(results[p], results[q]))
    out["bit_identical_b_vs_d"] = f"{same('b', 'd')}/{K}"
    out["bit_identical_a_vs_c"] = f"{same('a', 'c')}/{K}"
    out["max_abs_x_structured_minus_dense"] = max(float(np.abs(p[1] - q[1]).max()) for p, q in zip(results["a"], results["b"])
                                                  if p[1] is not None and q[1] is not None)
    for c in ctxs.values():
        c.close()
    print(json.dumps(out, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
