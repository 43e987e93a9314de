#!/usr/bin/env python
"""Measurements behind profiles/tall_batch.md (lockstep batches of tall LPs over one matrix).

32 members on one X (the generator of tests/test_gpu_tall_batches.py: planted optimal members), at (m_ub, nx) = (8192, 128)
and (4096, 512), default options.  One warm-up round, then five alternating rounds in one process; in each round
  (a) the 32 members one after another through Context.upload(problem, tall=True) + solve_raw     (the way before this entry)
  (b) upload_lockstep_shared_ub_eq + solve_lockstep                                               (m x m per member)
  (c) upload_lockstep_shared_ub_tall + solve_lockstep
Solves and uploads are timed separately (host clock; every call ends in a device synchronise); LP/s is 32 / the solve time.
Also: resident bytes of (b) and (c) and the phase split of one profiled solve of (c) (lpipm_set_profiling(1)).
  tall_batch_times.py [8192x128] [4096x512]     (default: both)        One JSON line on stdout."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lp_amd                      # noqa: E402

COUNT, ROUNDS = 32, 5


def shared_X(seed, m, nx):
    rng = np.random.default_rng(seed); X = rng.standard_normal((m, nx))
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


def shape(m, nx):
    X = shared_X(100 + m, m, nx)
    vec = [member(X, 1000 * m + i) for i in range(COUNT)]
    bs, cs = [v[0] for v in vec], [v[1] for v in vec]
    probs = [lp_amd.Problem.target(c).ub(X, b).build() for b, c in zip(bs, cs)]
    o = lp_amd.InteriorPoint.default().opts()
    ca, cb, cc = lp_amd.Context(0), lp_amd.Context(0), lp_amd.Context(0)

    def way_a():
        up = sv = 0.0
        res = []
        for p in probs:
            _, t = clock(lambda: ca.upload(p, tall=True)); up += t
            r, t = clock(lambda: ca.solve_raw(o)); sv += t
            res.append((r[0], r[3]))
        return up, sv, res

    def way_batch(cx, upload):
        _, up = clock(upload)
        r, sv = clock(lambda: cx.solve_lockstep(o))
        return up, sv, [(x[0], x[3]) for x in r]

    way_b = lambda: way_batch(cb, lambda: cb.upload_lockstep_shared_ub_eq(X, None, bs, cs))
    way_c = lambda: way_batch(cc, lambda: cc.upload_lockstep_shared_ub_tall(X, bs, cs))
    ways = (("a", way_a), ("b", way_b), ("c", way_c))
    warm = {k: f() for k, f in ways}                                   # code objects loaded, clocks up, allocations made
    out = {"members": COUNT, "status_iterations": {k: sorted(set(v[2])) for k, v in warm.items()},
           "same_status_and_iterations": warm["a"][2] == warm["b"][2] == warm["c"][2],
           "resident_bytes": {"b": cb.resident_bytes(), "c": cc.resident_bytes()}, "rounds": []}
    for _ in range(ROUNDS):
        row = {}
        for k, f in ways:
            up, sv, _ = f()
            row[k] = {"upload_s": up, "solve_s": sv, "lp_per_s": COUNT / sv}
        out["rounds"].append(row)
    med = lambda k, key: float(np.median([r[k][key] for r in out["rounds"]]))
    out["median"] = {k: {"upload_s": med(k, "upload_s"), "solve_s": med(k, "solve_s"), "lp_per_s": med(k, "lp_per_s")} for k, _ in ways}
    out["c_faster_than_a_in_every_round"] = all(r["c"]["solve_s"] < r["a"]["solve_s"] for r in out["rounds"])
    cc.set_profiling(1)
    cc.solve_lockstep(o)
    out["phases_c"] = cc.phase_times()
    cc.set_profiling(0)
    ca.upload(probs[0], tall=True)
    ca.set_profiling(1)
    ca.solve_raw(o)
    out["phases_a_one_member"] = ca.phase_times()
    for cx in (ca, cb, cc):
        cx.close()
    return out


if __name__ == "__main__":
    todo = sys.argv[1:] or ["8192x128", "4096x512"]
    print(json.dumps({s: shape(*[int(v) for v in s.split("x")]) for s in todo}))
