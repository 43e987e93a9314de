#!/usr/bin/env python
"""Measurements behind profiles/tall_own_batch.md (lockstep batches of tall LPs that own their matrices).

32 members, each with its own X (the generator of tests/test_gpu_tall_own_batches.py: planted optimal members), at
(m_ub, nx) = (8192, 128) and (4096, 512), default options.  One warm-up round, then five alternating rounds in one process; in
each round, WHOLE calls, uploads included:
  (a) the 32 members one after another through Context.upload(problem, tall=True) + solve_raw
  (b) Context.solve_batch on [X_i I] with the hint n_slack = m_ub (lpipm_solve_batch_slack: lockstep chunks, m x m per member)
  (c) Context.solve_batch(problems, tall=True)                    (lpipm_solve_batch_ub_tall)
and, apart, (r) the resident batch: upload_lockstep_ub_tall, then solve_lockstep alone.
Host clock; every call ends in a device synchronise; LP/s is 32 / the time of the whole call (of (r): of the solve alone).
Also: resident bytes of (r) and the phase split of one profiled solve of (r) and of one member alone (lpipm_set_profiling(1)).
  tall_own_batch_times.py [8192x128] [4096x512] [--skip-b]     (default: both shapes)        One JSON line on stdout."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lp_amd                      # noqa: E402

COUNT, ROUNDS = 32, 5


def own_X(seed, m, nx):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    X[0, :] = np.abs(X[0, :]); X[:, 0] = -np.abs(X[:, 0]); X[0, 0] = 0.0
    return X


def member(X, seed):
    rng = np.random.default_rng(seed)
    m, nx = X.shape
    k = nx // 2
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:k]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, k)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    return b, -X.T @ lam + mu


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return out, time.perf_counter() - t0


def shape(m, nx, with_b):
    Xs = [own_X(7000 + 37 * m + i, m, nx) for i in range(COUNT)]
    vec = [member(X, 1000 * m + i) for i, X in enumerate(Xs)]
    bs, cs = [v[0] for v in vec], [v[1] for v in vec]
    probs = [lp_amd.Problem.target(c).ub(X, b).build() for X, b, c in zip(Xs, bs, cs)]
    o = lp_amd.InteriorPoint.default().opts()
    ca, cb, cc, cr = lp_amd.Context(0), lp_amd.Context(0), lp_amd.Context(0), lp_amd.Context(0)
    slack = None
    if with_b:                                                         # [X_i I] on the host: what (b)'s caller has to hold
        eye = np.eye(m)
        slack = [(np.hstack([X, eye]), b, np.concatenate([c, np.zeros(m)]), 0.0, m) for X, b, c in zip(Xs, bs, cs)]

    def way_a():
        res = []
        for p in probs:
            ca.upload(p, tall=True)
            r = ca.solve_raw(o)
            res.append((r[0], r[3]))
        return res

    way_b = lambda: [(r[0], r[3]) for r in cb.solve_batch(slack, o)]
    way_c = lambda: [(r[0], r[3]) for r in cc.solve_batch(probs, o, tall=True)]
    ways = [("a", way_a), ("c", way_c)] + ([("b", way_b)] if with_b else [])

    def resident():
        _, up = clock(lambda: cr.upload_lockstep_ub_tall(Xs, bs, cs))
        r, sv = clock(lambda: cr.solve_lockstep(o))
        return up, sv, [(x[0], x[3]) for x in r]

    warm = {k: f() for k, f in ways}                                   # code objects loaded, clocks up, allocations made
    warm["r"] = resident()[2]
    out = {"members": COUNT, "status_iterations": {k: sorted(set(v)) for k, v in warm.items()},
           "same_status_and_iterations_as_a": {k: v == warm["a"] for k, v in warm.items() if k != "a"},
           "resident_bytes": {"r": cr.resident_bytes()}, "rounds": []}
    for _ in range(ROUNDS):
        row = {}
        for k, f in ways:
            _, t = clock(f)
            row[k] = {"call_s": t, "lp_per_s": COUNT / t}
        up, sv, _ = resident()
        row["r"] = {"upload_s": up, "solve_s": sv, "lp_per_s": COUNT / sv}
        out["rounds"].append(row)
    med = lambda k, key: float(np.median([r[k][key] for r in out["rounds"]]))
    out["median"] = {k: {key: med(k, key) for key in out["rounds"][0][k]} for k in out["rounds"][0]}
    out["c_faster_than_a_in_every_round"] = all(r["c"]["call_s"] < r["a"]["call_s"] for r in out["rounds"])
    cr.set_profiling(1)
    cr.solve_lockstep(o)
    out["phases_r"] = cr.phase_times()
    cr.set_profiling(0)
    ca.upload(probs[0], tall=True)
    ca.set_profiling(1)
    ca.solve_raw(o)
    out["phases_a_one_member"] = ca.phase_times()
    for cx in (ca, cb, cc, cr):
        cx.close()
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    todo = args or ["8192x128", "4096x512"]
    print(json.dumps({s: shape(*[int(v) for v in s.split("x")], "--skip-b" not in sys.argv) for s in todo}))
