"""What lpipm_get_certificate[_device] costs beside a solve (profiles/certificates.md): 32 shared-matrix members of 1024 x 2048,
4 of them made infeasible, one lpipm_solve_lockstep with profiling on, then the getter on the same context.  The getter is
synchronous, so each call is bracketed by two HIP events recorded on an otherwise idle stream.  The shared matrix is
planted_scenarios' with the extra row (0, 1, ..., 1) and a zero column 0, so that a member becomes infeasible through b alone
(last entry -1) and unbounded through c alone (c[0] = -1): one member is unbounded, too.  Prints one JSON line; --out FILE also
writes it there.

    python scripts/certificates_cost.py [--out FILE]"""
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
INFEASIBLE_MEMBERS, UNBOUNDED_MEMBER = (1, 9, 17, 25), 31
A0 = synth.planted_lp(5, m - 1, n)[0]
A = np.vstack([A0, np.ones(n)])
A[:, 0] = 0.0
rng = np.random.default_rng([5, m, n, K])
bs, cs = [], []
for k in range(K):
    basis = 1 + rng.permutation(n - 1)[:m]
    x, z = np.zeros(n), 1.0 + rng.random(n)
    x[basis] = 1.0 + rng.random(m); z[basis] = 0.0
    b, c = A @ x, A.T @ rng.standard_normal(m) + z
    if k in INFEASIBLE_MEMBERS:
        b[m - 1] = -1.0
    if k == UNBOUNDED_MEMBER:
        c[0] = -1.0
    bs.append(b); cs.append(c)
cx = lp_amd.Context(0)
cx.upload_lockstep_shared(A, bs, cs)
opts = lp_amd.InteriorPoint.default().opts()
cx.set_profiling(1)
res = cx.solve_lockstep(opts)
times = cx.phase_times()
iterations = max(r[3] for r in res)
yd = torch.empty((K, m), dtype=torch.float64, device="cuda")
cd = torch.empty((K, n), dtype=torch.float64, device="cuda")
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


infos = cx.certificates_device(yd.data_ptr(), m, cd.data_ptr(), n)
dev_ms, dev_wall = timed(lambda: cx.certificates_device(yd.data_ptr(), m, cd.data_ptr(), n))
one_ms, one_wall = timed(lambda: cx.certificate(INFEASIBLE_MEMBERS[0]))
none_ms, none_wall = timed(lambda: cx.certificate(0))
all_ms, all_wall = timed(lambda: cx.certificates_lockstep(), reps=5)
duals_ms, duals_wall = timed(lambda: cx.duals_device(yd.data_ptr(), m, cd.data_ptr(), n))
# one iteration's passes over A beside the getter's one: the residual pair's dual pass alone, on the same resident batch
out = dict(members=K, m=m, n=n, statuses=[r[0] for r in res], iterations=[r[3] for r in res],
           kinds=[d["kind"] for d in infos], residuals=[d["residual"] for d in infos if d["kind"]],
           solve_total_ms=times["total_ms"], solve_gemv_ms=times.get("gemv_ms"), solve_vec_ms=times["vec_ms"],
           solve_gemv_passes=times.get("gemv_passes"), solve_loop_iterations=iterations,
           get_certificate_device_ms=dev_ms, get_certificate_device_wall_ms=dev_wall,
           get_certificate_one_member_ms=one_ms, get_certificate_one_member_wall_ms=one_wall,
           get_certificate_member_without_ms=none_ms, get_certificate_member_without_wall_ms=none_wall,
           certificates_lockstep_all_members_host_ms=all_ms, certificates_lockstep_all_members_host_wall_ms=all_wall,
           get_duals_device_ms=duals_ms, get_duals_device_wall_ms=duals_wall)
print(json.dumps(out))
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
        json.dump(out, f, indent=1)
cx.close()
