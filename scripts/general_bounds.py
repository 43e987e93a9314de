"""The same LP with free columns through lpipm_upload_bounds and through the explicit split (every free column twice, once
negated, through lpipm_upload_ub_eq): whole-solve wall time, phase times, iteration counts and resident bytes -- the numbers
of profiles/general_bounds.md.

    python scripts/general_bounds.py [--repeats 10] [--out FILE] [--md FILE]

Every structural column is free.  A vertex of such an LP needs as many active rows as it has free columns, so the planted LP
has nx - m_eq `ub` rows beside its m_eq `eq` rows (tests/test_bounds_host.py's generator; all of them active).  Wall time: a
host clock around Context.solve_raw, which ends in a device synchronise, profiling off, the two uploads alternating, after two
warm-up solves each; the median and the extremes over the repeats -- the spread of the explicit split is what the new form
is judged against.  Phase times: one further solve each with lpipm_set_profiling(1)."""
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
    from test_bounds_host import explicit_parts, planted_bounds
    lp = planted_bounds(100 + m_eq, nx - m_eq, m_eq, nx, 0, 1, 0)
    A_ub, b_ub, A_eq, b_eq, c, lower, upper, _ = lp
    free = lp_amd.Problem.target(c).ub(A_ub, b_ub).eq(A_eq, b_eq).lower(lower).upper(upper).build()
    Au, bu, Ae, be, ce = explicit_parts(lp[:7])
    split = lp_amd.Problem.target(ce).ub(Au, bu).eq(Ae, be).build()
    return free, split


def net(name, x, nx):
    return x[:nx] if name == "bounds" else x[:nx] - x[nx: 2 * nx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import lp_amd
    opts = lp_amd.InteriorPoint.default().opts()
    rows = []
    for m_eq, nx in SHAPES:
        ctxs = {}
        for name, prob in zip(("bounds", "split"), problems(m_eq, nx)):
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
        dx = float(np.abs(net("bounds", ctxs["bounds"][1][1], nx) - net("split", ctxs["split"][1][1], nx)).max())
        for name, (cx, warm) in ctxs.items():
            cx.set_profiling(1)
            cx.solve_raw(opts)
            row = dict(shape=f"m_ub={nx - m_eq} m_eq={m_eq} nx={nx} nf={nx}", upload=name, status=warm[0], iterations=warm[3],
                       fun=warm[2], wall_ms_median=float(np.median(wall[name])), wall_ms_min=min(wall[name]),
                       wall_ms_max=max(wall[name]), resident_bytes=cx.resident_bytes(), phase_times=cx.phase_times(),
                       max_dx_net_between_uploads=dx)
            rows.append(row)
            print(json.dumps(row), flush=True)
            cx.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
    if args.md:
        keys = ("adat_ms", "potrf_ms", "trsv_ms", "gemv_ms", "vec_ms", "total_ms")
        with open(args.md, "w") as f:
            f.write("| shape | upload | status | iterations | wall ms median (min .. max) | resident MiB | "
                    + " | ".join(keys) + " |\n|---|---|---|---|---|---|" + "---|" * len(keys) + "\n")
            for r in rows:
                f.write(f"| {r['shape']} | {r['upload']} | {r['status']} | {r['iterations']} | {r['wall_ms_median']:.3f} "
                        f"({r['wall_ms_min']:.3f} .. {r['wall_ms_max']:.3f}) | {r['resident_bytes'] / 2 ** 20:.1f} | "
                        + " | ".join(f"{r['phase_times'][k]:.3f}" for k in keys) + " |\n")


if __name__ == "__main__":
    main()
