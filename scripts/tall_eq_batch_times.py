#!/usr/bin/env python
"""Measurements behind profiles/tall_eq_batch.md (lockstep batches of tall LPs with equality rows over one image).

32 members on one pair (X, A_eq) (the generator of tests/test_tall_eq_batch_host.py: planted optimal members) at
(m_ub, nx, m_eq) = (4096, 256, 16) and (8192, 128, 8), default options.  One warm-up round, then five alternating rounds in one
process; in each round
  (a)  the resident batch of upload_lockstep_shared_ub_eq_tall: solve_lockstep only, ten solves back to back per round (one
       solve is ~10 ms: too short a window for a host clock) and their mean; its one upload is timed before the rounds
  (b)  the same members one by one on one context through upload_tall_eq + solve_raw, uploads and solves timed apart: the
       resident solves alone (lp_per_s) and with their uploads (lp_per_s_with_uploads)
  (c)  upload_lockstep_shared_ub_eq (m x m per member), solve_lockstep only; left out with --no-dense
Three contexts in the process, no more: with one context per member (32 more streams and side streams on four hardware queues)
solves of every way stalled by ~10 ms now and then.  Host clock around calls that end in a device synchronise; LP/s is 32 / the
solve time.  Beside each: lpipm_get_resident_bytes, and the members' (status, iterations).  Also the phase split of one profiled
solve of (a) and of one optimal member of (b).
  tall_eq_batch_times.py [4096x256+16] [8192x128+8] [--no-dense]     (default: both shapes)        One JSON line on stdout."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lp_amd                                                  # noqa: E402
from test_tall_eq_batch_host import member, shared_pair        # noqa: E402

COUNT, ROUNDS, REPS_A = 32, 5, 10


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def shape(m, nx, me, dense):
    X, Ae = shared_pair(100 + m + me, m, nx, me)
    vec = [member(X, Ae, 1000 * m + 10 * me + i) for i in range(COUNT)]
    bs, cs = [np.concatenate([v[0], v[1]]) for v in vec], [v[2] for v in vec]
    probs = [lp_amd.Problem.target(c).ub(X, b[:m]).eq(Ae, b[m:]).build() for b, c in zip(bs, cs)]
    o = lp_amd.InteriorPoint.default().opts()
    ca, cu = lp_amd.Context(0), lp_amd.Context(0)
    _, up_a = clock(lambda: ca.upload_lockstep_shared_ub_eq_tall(X, Ae, bs, cs))
    cc = None
    if dense:
        cc = lp_amd.Context(0)
        cc.upload_lockstep_shared_ub_eq(X, Ae, bs, cs)

    def batch(cx, reps=1):
        r, sv = clock(lambda: [cx.solve_lockstep(o) for _ in range(reps)][-1])
        return 0.0, sv / reps, [(x[0], x[3]) for x in r]

    def way_b():
        up = sv = 0.0
        res = []
        for pr in probs:
            _, t = clock(lambda: cu.upload_tall_eq(pr)); up += t
            r, t = clock(lambda: cu.solve_raw(o)); sv += t
            res.append((r[0], r[3]))
        return up, sv, res

    ways = [("a", lambda: batch(ca, REPS_A)), ("b", way_b)] + ([("c", lambda: batch(cc))] if dense else [])
    warm = {k: f() for k, f in ways}                                   # code objects loaded, clocks up, allocations made
    out = {"members": COUNT, "status_iterations": {k: v[2] for k, v in warm.items()},
           "same_status_and_iterations": all(v[2] == warm["a"][2] for v in warm.values()),
           "upload_a_s": up_a,
           "resident_bytes": {"a": ca.resident_bytes(), "b_one_member": cu.resident_bytes(),
                              **({"c": cc.resident_bytes()} if dense else {})},
           "rounds": []}
    for _ in range(ROUNDS):
        row = {}
        for k, f in ways:
            up, sv, _ = f()
            row[k] = {"upload_s": up, "solve_s": sv, "lp_per_s": COUNT / sv, "lp_per_s_with_uploads": COUNT / (sv + up)}
        out["rounds"].append(row)
    med = lambda k, key: float(np.median([r[k][key] for r in out["rounds"]]))
    out["median"] = {k: {key: med(k, key) for key in ("upload_s", "solve_s", "lp_per_s", "lp_per_s_with_uploads")} for k, _ in ways}
    out["a_faster_than_b_in_every_round"] = all(r["a"]["solve_s"] < r["b"]["solve_s"] for r in out["rounds"])
    ca.set_profiling(1)
    ca.solve_lockstep(o)
    out["phases_a"] = ca.phase_times()
    cu.upload_tall_eq(probs[[st for st, _ in warm["b"][2]].index(0)])  # an optimal member
    cu.set_profiling(1)
    cu.solve_raw(o)
    out["phases_b_one_member"] = cu.phase_times()
    for cx in [ca, cu] + ([cc] if dense else []):
        cx.close()
    return out


if __name__ == "__main__":
    dense = "--no-dense" not in sys.argv[1:]
    todo = [a for a in sys.argv[1:] if not a.startswith("--")] or ["4096x256+16", "8192x128+8"]
    res = {}
    for s in todo:
        mn, me = s.split("+")
        m, nx = mn.split("x")
        res[s] = shape(int(m), int(nx), int(me), dense)
    print(json.dumps(res))
