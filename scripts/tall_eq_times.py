#!/usr/bin/env python
"""Measurements behind profiles/tall_eq.md (tall LPs with equality rows).

One planted LP per shape (the generator of tests/test_tall_eq_host.py) at (m_ub, nx, m_eq) = (4096, 256, 16) and
(16384, 512, 64), default options, three resident problems on three contexts:
  (a) Context.upload(problem)             lpipm_upload_ub_eq: the m x m normal matrix, m = m_ub + m_eq
  (b) Context.upload_tall_eq(problem)     lpipm_upload_ub_eq_tall: K on the `ub` rows, Schur complement for the `eq` rows
  (c) Context.upload(ub rows, tall=True)  lpipm_upload_ub_tall on the same X without the `eq` rows: what (b) can at best reach
One warm-up solve each, then five alternating rounds in one process; solves only (the uploads are made once, before), host
clock around solve_raw, which ends in a device synchronise.  Also: resident bytes, and the phase split of one profiled solve
of each (lpipm_set_profiling(1)): potrf_ms(b) - potrf_ms(c) is Zt, S and its factorisation, trsv_ms(b) - trsv_ms(c) the
split solve with the two solves on S, gemv_ms(b) - gemv_ms(c) the two passes over Zt.
  tall_eq_times.py [4096x256+16] [16384x512+64]      (default: both shapes)        One JSON line on stdout."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lp_amd                                  # noqa: E402
from test_tall_eq_host import planted_eq       # noqa: E402

ROUNDS = 5


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def shape(m, nx, me):
    X, b, Ae, be, c, xs = planted_eq(1, m, nx, me)
    full = lp_amd.Problem.target(c).ub(X, b).eq(Ae, be).build()
    ub_only = lp_amd.Problem.target(c).ub(X, b).build()
    o = lp_amd.InteriorPoint.default().opts()
    cxs = {"a": lp_amd.Context(0), "b": lp_amd.Context(0), "c": lp_amd.Context(0)}
    cxs["a"].upload(full)
    cxs["b"].upload_tall_eq(full)
    cxs["c"].upload(ub_only, tall=True)
    warm = {k: cx.solve_raw(o) for k, cx in cxs.items()}
    out = {"status_iterations": {k: (r[0], r[3]) for k, r in warm.items()},
           "b_vs_a_max_dx": float(np.abs(warm["b"][1] - warm["a"][1]).max()),
           "b_vs_planted_max_dx": float(np.abs(warm["b"][1][:nx] - xs).max()),
           "resident_bytes": {k: cx.resident_bytes() for k, cx in cxs.items()}, "rounds": []}
    for _ in range(ROUNDS):
        out["rounds"].append({k: clock(lambda: cx.solve_raw(o))[1] for k, cx in cxs.items()})
    out["median_s"] = {k: float(np.median([r[k] for r in out["rounds"]])) for k in cxs}
    out["b_faster_than_a_in_every_round"] = all(r["b"] < r["a"] for r in out["rounds"])
    out["phases"] = {}
    for k, cx in cxs.items():
        cx.set_profiling(1)
        cx.solve_raw(o)
        out["phases"][k] = cx.phase_times()
        cx.close()
    return out


if __name__ == "__main__":
    todo = [a for a in sys.argv[1:] if not a.startswith("--")] or ["4096x256+16", "16384x512+64"]
    res = {}
    for s in todo:
        mn, me = s.split("+")
        m, nx = mn.split("x")
        res[s] = shape(int(m), int(nx), int(me))
    print(json.dumps(res))
