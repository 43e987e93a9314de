#!/usr/bin/env python3
"""A sweep of --count scenarios (default 256) over ONE planted 1024x2048 matrix (synth.planted_scenarios), in lockstep groups of
--max-group (default 32), wall clock including every upload:
  (a) reupload : lp_amd.batch.solve_shared_matrix -- one lpipm_upload_lockstep_shared per chunk (A again, the context laid out
                 again, the first iteration's factor formed again), and
  (b) sweep    : lp_amd.batch.sweep_shared_matrix -- one upload, lpipm_update_lockstep_vectors per later chunk.
--runs alternating runs of each (after one unrecorded run of each), LP/s per run and their medians; every member of (b) is
compared with (a) bit for bit.  Then, for one resident shared batch of --max-group members with the first-factor cache on and
off (off is the behaviour before the one shared factor): resident bytes, the first solve after a fresh upload (median of
--runs fresh contexts) and the per-lockstep-iteration phase split of a profiled later solve (lpipm_set_profiling(1))."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _same(a, b):
    return (a["status"] == b["status"] and a["iterations"] == b["iterations"] and a["fun"] == b["fun"]
            and (a["x_slack"] is None) == (b["x_slack"] is None)
            and (a["x_slack"] is None or a["x_slack"].tobytes() == b["x_slack"].tobytes()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--max-group", type=int, default=32)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import lp_amd
    from lp_amd import batch, synth
    A, bs, cs, _ = synth.planted_scenarios(0, args.m, args.n, args.count)
    o = lp_amd.InteriorPoint.default().opts()
    ways = {"reupload": batch.solve_shared_matrix, "sweep": batch.sweep_shared_matrix}
    ctx = {name: lp_amd.Context(0) for name in ways}
    rates = {name: [] for name in ways}
    last = {}
    for run in range(args.runs + 1):                     # run 0 warms both up and is not recorded
        for name, fn in ways.items():
            t0 = time.perf_counter()
            last[name] = fn(A, bs, cs, opts=o, ctx=ctx[name], max_group=args.max_group)
            dt = time.perf_counter() - t0
            if run:
                rates[name].append(round(args.count / dt, 1))
    for c in ctx.values():
        c.close()
    same = [_same(a, b) for a, b in zip(last["reupload"], last["sweep"])]
    out = dict(count=args.count, max_group=args.max_group, shape=[args.m, args.n],
               lp_per_s={k: v for k, v in rates.items()},
               lp_per_s_median={k: float(np.median(v)) for k, v in rates.items()},
               every_sweep_run_above_every_reupload_run=min(rates["sweep"]) > max(rates["reupload"]),
               members_bit_identical=f"{sum(same)}/{args.count}",
               members_ok=sum(r["status"] == 0 for r in last["sweep"]))
    g = min(args.max_group, args.count)
    for name, on in (("cache_on", True), ("cache_off", False)):
        first = []
        for _ in range(args.runs):
            c = lp_amd.Context(0).set_first_factor_cache(on)
            c.upload_lockstep_shared(A, bs[:g], cs[:g])
            t0 = time.perf_counter()
            c.solve_lockstep(o)
            first.append(time.perf_counter() - t0)
            resident = c.resident_bytes()
            c.close()
        c = lp_amd.Context(0).set_first_factor_cache(on)
        c.upload_lockstep_shared(A, bs[:g], cs[:g])
        c.solve_lockstep(o)
        c.set_profiling(1)
        c.solve_lockstep(o)
        pt = c.phase_times()
        c.close()
        it = max(pt["iterations"], 1)
        out[name] = dict(resident_bytes=resident, first_solve_ms=[round(1e3 * t, 3) for t in first],
                         first_solve_ms_median=round(1e3 * float(np.median(first)), 3),
                         later_solve_per_iteration_ms={k: round(pt[k + "_ms"] / it, 4) for k in ("adat", "potrf", "trsv", "gemv", "vec", "total")},
                         later_solve_trsv_ms=round(pt["trsv_ms"], 4),      # (the two differ in iteration 1's solves alone)
                         later_solve_iterations=int(pt["iterations"]), later_solve_adat_launches=int(pt["adat_launches"]))
    out["one_shared_set_bytes"] = out["cache_on"]["resident_bytes"] - out["cache_off"]["resident_bytes"]
    print(json.dumps(out, indent=1))
    return 0 if all(same) else 1


if __name__ == "__main__":
    sys.exit(main())
