"""The same bounded LP through lpipm_upload_bounded and through the explicit upload (its bounds as `ub` rows, lpipm_upload_ub_eq):
whole-solve wall time, phase times, iteration counts and resident bytes -- the numbers of profiles/bounded_form.md.

    python scripts/bounded_form.py [--repeats 10] [--out FILE]

Every column is bounded.  Wall time: a host clock around Context.solve_raw, which ends in a device synchronise, profiling off,
the two uploads alternating, after two warm-up solves each; the median and the extremes over the repeats.  Phase times: one
further solve each with lpipm_set_profiling(1).  The LPs are tests/test_bounded_host.py's planted vertices."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = [(1024, 2048), (512, 1024)]          # (m_eq, nx)


def problems(m_eq, nx):
    import lp_amd
    from test_bounded_host import explicit_parts, planted_box
    A_ub, b_ub, A_eq, b_eq, c, u, _ = planted_box(100 + m_eq, 0, m_eq, nx, 1, .5)
    bounded = lp_amd.Problem.target(c).eq(A_eq, b_eq).upper(u).build()
    Au, bu = explicit_parts(A_ub, b_ub, u)
    explicit = lp_amd.Problem.target(c).ub(Au, bu).eq(A_eq, b_eq).build()
    return bounded, explicit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import lp_amd
    opts = lp_amd.InteriorPoint.default().opts()
    rows = []
    for m_eq, nx in SHAPES:
        ctxs = {}
        for name, prob in zip(("bounded", "explicit"), problems(m_eq, nx)):
            cx = lp_amd.Context(0)
            cx.upload(prob)
            for _ in range(2):
                warm = cx.solve_raw(opts)
            ctxs[name] = (cx, warm)
        wall = {name: [] for name in ctxs}
        for _ in range(args.repeats):
            for name, (cx, _) in ctxs.items():
                t0 = time.perf_counter()
                cx.solve_raw(opts)
                wall[name].append((time.perf_counter() - t0) * 1e3)
        dx = float(np.abs(ctxs["bounded"][1][1] - ctxs["explicit"][1][1]).max())
        for name, (cx, warm) in ctxs.items():
            cx.set_profiling(1)
            cx.solve_raw(opts)
            row = dict(shape=f"m_eq={m_eq} nx={nx} nb={nx}", upload=name, status=warm[0], iterations=warm[3], fun=warm[2],
                       wall_ms_median=float(np.median(wall[name])), wall_ms_min=min(wall[name]), wall_ms_max=max(wall[name]),
                       resident_bytes=cx.resident_bytes(), phase_times=cx.phase_times(), max_dx_between_uploads=dx)
            rows.append(row)
            print(json.dumps(row), flush=True)
            cx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
