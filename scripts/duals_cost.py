"""What lpipm_get_duals[_device] costs beside a solve (profiles/duals.md): 32 shared-matrix members of 1024 x 2048, one
lpipm_solve_lockstep with profiling on, then the getter on the same context.  The getter is synchronous, so each call is
bracketed by two HIP events recorded on an otherwise idle stream.  Prints one JSON line; --out FILE also writes it there.

    python scripts/duals_cost.py [--out FILE]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lp_amd
from lp_amd import synth

K, m, n = 32, 1024, 2048
A, bs, cs, _ = synth.planted_scenarios(5, m, n, K)
cx = lp_amd.Context(0)
cx.upload_lockstep_shared(A, bs, cs)
opts = lp_amd.InteriorPoint.default().opts()
cx.set_profiling(1)
res = cx.solve_lockstep(opts)
times = cx.phase_times()
yd = torch.empty((K, m), dtype=torch.float64, device="cuda")
zd = torch.empty((K, n), dtype=torch.float64, device="cuda")
torch.cuda.synchronize()


def timed(fn, reps=20):
    fn()                                  # the staging block is made at first use
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out, wall = [], []
    for _ in range(reps):
        ev[0].record(); t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3); ev[1].record(); ev[1].synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out)), float(np.median(wall))


dev_ms, dev_wall = timed(lambda: cx.duals_device(yd.data_ptr(), m, zd.data_ptr(), n))
one_ms, one_wall = timed(lambda: cx.duals(0))
all_ms, all_wall = timed(lambda: cx.duals_lockstep(), reps=5)
each_ms, each_wall = timed(lambda: [cx.duals(k) for k in range(K)], reps=5)
out = dict(members=K, m=m, n=n, statuses=sorted(set(r[0] for r in res)), iterations=sorted(set(r[3] for r in res)),
           solve_total_ms=times["total_ms"], solve_vec_ms=times["vec_ms"],
           get_duals_device_ms=dev_ms, get_duals_device_wall_ms=dev_wall,
           get_duals_one_member_ms=one_ms, get_duals_one_member_wall_ms=one_wall,
           duals_lockstep_all_members_host_ms=all_ms, duals_lockstep_all_members_host_wall_ms=all_wall,
           get_duals_32_calls_host_ms=each_ms, get_duals_32_calls_host_wall_ms=each_wall)
print(json.dumps(out))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
cx.close()
