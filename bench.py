#!/usr/bin/env python3
"""bench.py -- IPM iterations/sec on the headline workload of BASELINE.json (dense 4096x8192 fp64 LP).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  (N > 1: launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...`)

A "step" is one complete `InteriorPoint::solve` (mod.rs:199-240) of the rank's LP: the whole hot path
(A.D.A^T, Cholesky, triangular solves, GEMVs, vector kernels) for as many IPM iterations as the
solver needs, with A already resident in HBM (uploaded once before the timed region).
Weak scaling: every rank owns ONE independent LP of the same shape (seed = rank) -- the batch shards
one per GPU with no data-path collective -- and the timed region ends with the single RCCL
all-gather of the solutions.  value = IPM iterations of all ranks / max-over-ranks wall time.

A plain run does only what `value` needs: it sets up, runs the W warm-up and K timed steps, writes the outputs of the
last timed step if --dump-outputs is given and prints the JSON line (with the `roofline` object, whose figures come from
the events recorded inside the timed region).  On the default workload --dump-outputs also runs the short c2 and c4
steps, for their outputs alone.  --full adds, after the timed region, everything else the benchmark
measures or checks: the per-phase breakdown, the unbracketed pass, the distance to the planted optimum, the CPU baselines,
the c4 parity check and, on the default workload, the c2 and c4 measurements.  The timed steps are the same in both.

`--workload c2` (optional): BASELINE config 2 -- one 512x1024 LP per GPU ("GEMV-bound, HBM roofline check"), same
protocol; its `roofline` object is the HBM one: the passes over A (GEMV-N / GEMV-T), algorithmic bytes 8mn per pass /
the average pass duration from HIP events on the solver's stream inside the timed region, against 8 TB/s.
`--workload c4` (optional): BASELINE config 4 -- 32 independent 1024x2048 LPs per GPU as one lockstep batch with
resident inputs, value in LP/s; same timing protocol; its `roofline` is the whole-solve MFMA fraction (+ with --full the
batched A.D.A^T launch's own); with --full it exits non-zero if a member lies outside the oracle's own envelope on that
LP widened by 1e-6 or takes an iteration count the oracle never produced (tests/golden/make_envelopes.py).
With --full the default workload (no --workload) measures the headline C3 and then, briefly, c2 and c4 as well: they are
appended to the one JSON line as the objects "c2" and "c4" (`value` stays the headline's); --only-headline skips them.

Objects on the JSON line besides the headline figures:
  roofline     : the dominant kernel (A.D.A^T, MFMA-bound): algorithmic flops m(m+1)n per launch /
                 its average launch duration from HIP events recorded on the solver's own stream
                 INSIDE the timed region (2 events per iteration, bracketing that kernel and its fix-up);
                 peak = 78.6 TFLOP/s dense fp64 MFMA.
  --full only:
  phase_ms_per_iteration : from one extra, untimed solve with every phase bracketed.
  unbracketed  : the timed steps once more with no HIP event recorded inside a solve (`value` stays the bracketed run).
  cpu_baseline : rank 0, N == 1 only: the single-threaded C restatement of the reference (oracle/, kind "port") timed
                 on this box's host for the first TWO IPM iterations of the same LP (two runs, max_iter 1 and 2: the
                 second iteration's time is the difference; the op count does not depend on the iterate), plus
                 "strong": the NumPy/OpenBLAS transcription on all host cores (stand-in for the reference's
                 `openblas-system` feature, Cargo.toml:23-24).  Baselines, not targets.
  roofline.traffic / mfma_busy_pmc come from a separate rocprofv3 --pmc run (counters cannot be read from inside this
                 process) whose summary is committed under profiles/ WITH a hash of lp_amd/csrc at collection time:
                 they are reported only while that hash still matches the sources ("recorded, not measured in this run").

--dump-outputs DIR: after the run, rank 0 writes what the timed path returned in its LAST timed step as DIR/<name>.npy
(float64): x (the solution, or the gathered block of all ranks), fun, iterations, status; c4: one row / entry per member.
The default workload adds the same for its c2 / c4 steps as c2_<name> / c4_<name> (with or without --full; not with
--only-headline).  The inputs are seeded (synth.planted_lp), so two builds run with the same arguments can be compared
output by output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

_RESULT_FD = 1


def emit(obj):
    os.write(_RESULT_FD, (json.dumps(obj) + "\n").encode())


PEAK_FP64_MFMA_TFLOPS = 78.6   # MI355X dense fp64 matrix peak (probe: lpipm_k_mfma_f64_probe ~76 TF/s)
PEAK_HBM_GBS = 8000.0          # HBM3E peak (MI355X_MICROARCH.md; ~6.3 TB/s achievable)


def csrc_hash() -> str:
    """sha256 over the kernel / host sources of liblpipm.so (what a PMC summary under profiles/ is stamped with)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "lp_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.hpp")) + glob.glob(os.path.join(d, "*.cpp"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, outputs, np):
    """--dump-outputs: every output of the last timed step as d/<name>.npy in float64."""
    if d is None:
        return
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes of outputs exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(d, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(d, k + ".npy"), a)


def cpu_baseline(A, b, c, m, n):
    """The reference's CPU path, restated (oracle/), timed on this box's host cores on a bounded sample of the same LP.
    port   : single-threaded C restatement with the reference's as-written op counts -- iterations 1 and 2
             (the default backend is single-threaded: ndarray without rayon/blas, Cargo.toml:31-33);
    strong : the NumPy/OpenBLAS transcription on all host cores (stand-in for `openblas-system`, Cargo.toml:23-24)."""
    from oracle import capi as oracle                        # checker / baseline only
    from oracle import oracle_np
    big = m * n >= 1 << 24
    t1 = time.perf_counter()
    r1 = oracle.solve(A, b, c, 0.0, oracle.default_opts(max_iter=1), want_log=False)
    r2 = oracle.solve(A, b, c, 0.0, oracle.default_opts(max_iter=2), want_log=False)
    tc = time.perf_counter() - t1
    it1 = r1["timing"]["total"]
    it2 = r2["timing"]["total"] - it1
    per_it = 0.5 * r2["timing"]["total"]
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:                                   # the threads OpenBLAS actually runs (it caps its pool below the affinity mask)
        from threadpoolctl import threadpool_info
        blas = [t["num_threads"] for t in threadpool_info() if t.get("user_api") == "blas"]
        if blas:
            ncores = min(ncores, max(blas))
    except Exception:
        pass
    k = 3 if big else 6
    t1 = time.perf_counter()
    rs = oracle_np.solve(A, b, c, 0.0, oracle_np.Opts(max_iter=k))
    ts = time.perf_counter() - t1
    return {
        "value": 1.0 / per_it, "unit": "iterations/s", "cores": 1, "kind": "port",
        "sample": f"IPM iterations 1 and 2 of the same {m}x{n} LP with the single-threaded C restatement of the reference "
                  f"(as-written op counts): {it1:.2f} s and {it2:.2f} s ({tc:.1f} s of CPU work in two runs, max_iter 1 and 2); "
                  f"the op count per iteration does not depend on the iterate",
        "seconds_iteration_1": it1, "seconds_iteration_2": it2,
        "phase_s_two_iterations": r2["timing"],
        "strong": {"value": rs.iterations / rs.timing["total"], "unit": "iterations/s", "cores": ncores,
                   "kind": "port-openblas",
                   "sample": f"{rs.iterations} iterations of the same LP with the NumPy/SciPy (OpenBLAS, LAPACK dpotrf/dpotrs) "
                             f"transcription on {ncores} host cores, {ts:.1f} s",
                   "phase_s": rs.timing},
    }



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 5; c2: 200)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float64); on the default workload also "
                         "those of the short c2 / c4 steps")
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also measure and check everything beyond the headline figure: per-phase "
                         "breakdown, unbracketed pass, planted-optimum distance, CPU baselines, c4 parity, and on the "
                         "default workload the c2 / c4 measurements")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--only-headline", action="store_true",
                    help="with --full: skip the short c2 / c4 measurements appended to the default workload")
    ap.add_argument("--workload", choices=("c3", "c2", "c4"), default="c3",
                    help="c3 (default, the BASELINE metric): one 4096x8192 LP per GPU; c2: one 512x1024 LP per GPU (HBM "
                         "roofline on the GEMV passes); c4: a shard of 32 independent 1024x2048 LPs per GPU as one lockstep "
                         "batch (BASELINE config 4: 256 LPs over 8 GPUs)")
    args = ap.parse_args()
    if args.workload == "c2":
        args.m, args.n = 512, 1024
    if args.steps is None:
        args.steps = 200 if args.workload == "c2" else 5   # a C2 solve is ~2 ms: keep the timed region near half a second
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # STDOUT carries exactly one line, the JSON result.  Libraries that print to file descriptor 1 on their own (RCCL's
    # version banner under NCCL_DEBUG=VERSION, warnings) are sent to stderr for the lifetime of the process.
    global _RESULT_FD
    sys.stdout.flush()
    _RESULT_FD = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run --nproc-per-node N")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import numpy as np
    import torch
    import lp_amd
    from lp_amd import synth

    dist = None
    if world > 1 or os.environ.get("LPIPM_BENCH_FORCE_DIST") == "1":   # the latter: rehearse the N>1 path on one GPU
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")          # only matter for the one-rank rehearsal:
        os.environ.setdefault("MASTER_PORT", "29517")              # torch.distributed.run sets both
        dist.init_process_group(backend="nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", local_rank)

    if args.workload == "c4":
        return bench_c4(args, rank, local_rank, world, dist, dev, np, torch, lp_amd, synth)
    env = (rank, local_rank, world, dist, dev, np, torch, lp_amd, synth)
    out, outputs = measure_single(args.m, args.n, args.steps, args.warmup, args.workload == "c2", args.full,
                                  args.full and world == 1 and not args.no_cpu_baseline, *env)
    nbad = 0
    if ((args.full or args.dump_outputs is not None) and args.workload == "c3" and (args.m, args.n) == (4096, 8192)
            and not args.only_headline):
        # The other two single-node configs of BASELINE.json, measured in the SAME run (short; after the headline's timed
        # region), so that a --full run records them too: c2 = config 2 (one 512x1024 LP per GPU, HBM roofline of the
        # passes over A), c4 = config 4 (32 LPs of 1024x2048 per GPU as one lockstep batch, LP/s, whole-solve MFMA
        # fraction, parity of every member against the oracle's envelope).  `value` above stays the headline's.
        # --dump-outputs without --full runs their steps too, for the c2_ / c4_ outputs alone (no object on the line).
        c2, c2_outputs = measure_single(512, 1024, 100, 5, True, args.full, False, *env)
        c4, nbad, c4_outputs = measure_c4(3, 1, args.full, *env)
        outputs.update({"c2_" + k: v for k, v in c2_outputs.items()})
        outputs.update({"c4_" + k: v for k, v in c4_outputs.items()})
        if rank == 0 and args.full:
            keep = ("metric", "value", "unit", "ms_per_step", "config", "roofline")
            out["c2"] = {k: c2[k] for k in keep}
            out["c2"]["phase_ms_per_iteration"] = c2["phase_ms_per_iteration"]
            out["c2"]["unbracketed"] = c2.get("unbracketed")
            out["c4"] = {k: c4[k] for k in keep}
            out["c4"]["phase_ms_per_lockstep_iteration"] = c4["phase_ms_per_lockstep_iteration"]
            out["c4"]["parity_rank0"] = c4["parity_rank0"]
            out["c4"]["parity_failed_members_any_rank"] = c4["parity_failed_members_any_rank"]
    if rank == 0:
        dump_outputs(args.dump_outputs, outputs, np)
        emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if nbad:
        sys.stderr.write(f"bench: {nbad} member(s) of the C4 shard outside the parity tolerance\n")
        sys.exit(1)


def measure_single(m, n, steps, warmup, c2, full, want_cpu_baseline, rank, local_rank, world, dist, dev, np, torch, lp_amd,
                   synth):
    """One independent m x n LP per GPU (seed = rank): the headline protocol (C3) and BASELINE config 2.  full: the untimed
    phase breakdown, unbracketed pass and planted-optimum distance after the timed region.  Returns (the result dict on
    rank 0 (None elsewhere), the outputs of the last timed step)."""
    A, b, c, xstar = synth.planted_lp(rank, m, n)        # one independent LP per rank (seed = rank)
    ctx = lp_amd.Context(local_rank)
    ctx.upload_arrays(A, b, c)                           # one-time H2D, outside the timed region
    solver = lp_amd.InteriorPoint.default()              # reference defaults (mod.rs:52-59)
    opts = solver.opts()
    x_dev = torch.zeros(n, dtype=torch.float64, device=dev)
    gathered = torch.zeros(world * n, dtype=torch.float64, device=dev) if dist is not None else None

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def one_step():
        rc, _, fun, its, _ = ctx.solve_raw(opts, x_dev_ptr=x_dev.data_ptr())
        if rc != 0:
            raise RuntimeError(f"solve failed with status {rc}")
        if dist is not None:                             # the single RCCL gather of the batch's solutions
            dist.all_gather_into_tensor(gathered, x_dev)
        return its, fun

    for _ in range(warmup):
        one_step()
    # HIP events recorded on the solver's own stream: c3 -- around the dominant kernel only (2 per iteration);
    # c2 -- every phase (the GEMV passes are five separate intervals per iteration)
    ctx.set_profiling(1 if c2 else 2)
    adat_ms = 0.0
    adat_launches = 0
    gemv_ms = 0.0
    gemv_passes = 0
    iters_local = 0
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        its, fun = one_step()
        iters_local += its
        pt = ctx.phase_times()
        adat_ms += pt["adat_ms"]
        adat_launches += pt["adat_launches"]
        gemv_ms += pt["gemv_ms"]
        gemv_passes += pt["gemv_passes"]
    barrier()
    dt = time.perf_counter() - t0
    # what the last timed step returned, before the solves below overwrite x_dev
    outputs = {"x": (gathered if dist is not None else x_dev).cpu().numpy(), "fun": fun, "iterations": its, "status": 0}
    phase = unbracketed = err = None
    if full:
        # per-phase breakdown: one more solve with every phase bracketed by events, OUTSIDE the timed region
        ctx.set_profiling(1)
        ctx.solve_raw(opts, x_dev_ptr=x_dev.data_ptr())
        pt = ctx.phase_times()
        phase = {k: pt[k] for k in ("adat_ms", "potrf_ms", "trsv_ms", "gemv_ms", "vec_ms", "total_ms")}
        phase_iters = max(int(pt["iterations"]), 1)
        ctx.set_profiling(0)
        # config 2 is a chain of ~30 launches of 5-30 us per iteration: the event brackets of its phase split cost a visible
        # share of it (at C3 the two events around A.D.A^T cost ~0.2 %).  The same steps once more with no event recorded at
        # all (every rank runs them: the step holds the gather); `value` stays the bracketed measurement above
        barrier()
        t1 = time.perf_counter()
        its_u = 0
        for _ in range(steps):
            its_u += one_step()[0]
        barrier()
        dt_u = time.perf_counter() - t1
        unbracketed = {"value": its_u / dt_u, "unit": "iterations/s (this rank)", "ms_per_step": dt_u * 1e3 / steps,
                       "ms_per_iteration": dt_u * 1e3 / max(its_u, 1),
                       "note": "the same steps with profiling off: no HIP event recorded inside a solve"}
        # parity guard on what was just solved: the planted vertex is the known answer
        err = float((x_dev.cpu().numpy() - xstar).__abs__().max())
    ctx.close()

    if dist is not None:
        t = torch.tensor([dt, float(iters_local)], dtype=torch.float64, device=dev)
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tsum = t.clone()
        dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
        dt_max, iters_total = float(tmax[0]), float(tsum[1])
    else:
        dt_max, iters_total = dt, float(iters_local)
    if rank != 0:
        return None, outputs
    flops_per_launch = float(m) * (m + 1) * n                     # lower triangle of A.D.A^T
    avg_ms = adat_ms / max(adat_launches, 1)
    achieved = flops_per_launch / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
    # HBM-side bytes per launch come from a separate rocprofv3 --pmc run (counters cannot be read from inside this
    # process).  The committed summary carries the hash of lp_amd/csrc it was collected with; a stale one is not used.
    traffic = None
    mfma_busy = None
    pmc_note = "no PMC summary for this workload"
    pmc_path = os.path.join(ROOT, "profiles", "r03_gemv_pmc.json" if c2 else "r03_adat_pmc.json")
    if (m, n) in ((4096, 8192), (512, 1024)) and os.path.exists(pmc_path):
        pmc = json.load(open(pmc_path))
        if pmc.get("csrc_sha256") == csrc_hash():
            traffic = pmc.get("traffic_bytes_per_launch")
            mfma_busy = pmc.get("mfma_busy_fraction")
            pmc_note = f"recorded by rocprofv3 --pmc ({os.path.relpath(pmc_path, ROOT)}), not measured in this run; kernel sources unchanged since"
        else:
            pmc_note = f"{os.path.relpath(pmc_path, ROOT)} was collected with other kernel sources (hash mismatch): not reported"
    if c2:
        bytes_per_pass = 8.0 * m * n                               # A once per pass (1 or 2 vectors ride along)
        avg_ms = gemv_ms / max(gemv_passes, 1)
        achieved = bytes_per_pass / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
        roofline = {"kernel": "gemv_n_kernel / gemv_t_kernel (passes over A: A.w and A^T.v, 1-2 vectors per pass)",
                    "bound": "hbm", "achieved": achieved, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                    "frac": achieved / PEAK_HBM_GBS, "traffic": traffic, "traffic_note": pmc_note,
                    "algorithmic_bytes_per_launch": bytes_per_pass, "avg_launch_ms": avg_ms, "launches": gemv_passes,
                    "note": "at this size a pass moves 4 MiB: its duration is the dependent-dispatch latency of a kernel, "
                            "not bytes (DESIGN.md 3.4)"}
    else:
        roofline = {"kernel": "gemm_nt_units_kernel<false> (A.diag(x/z).A^T as (tile, chunk) units with the in-launch combine, "
                              "lower 128x128 tiles, blocks above the diagonal left out, v_mfma_f64_16x16x4_f64)",
                    "bound": "mfma", "achieved": achieved, "peak": PEAK_FP64_MFMA_TFLOPS,
                    "unit": "TFLOP/s", "frac": achieved / PEAK_FP64_MFMA_TFLOPS,
                    "traffic": traffic, "traffic_unit": "bytes/launch (PMC FETCH_SIZE x2 + WRITE_SIZE)",
                    "traffic_note": pmc_note,
                    "algorithmic_bytes_per_launch": 8.0 * m * n + 4.0 * m * m,
                    "mfma_busy_pmc": mfma_busy,   # SQ_VALU_MFMA_BUSY_CYCLES share of the kernel's SIMD-cycles (same JSON)
                    "avg_launch_ms": avg_ms, "launches": adat_launches,
                    "flops_per_launch": flops_per_launch}
    out = {
        "metric": f"IPM iterations/sec, dense {m}x{n} fp64 LP",
        "value": iters_total / dt_max,
        "unit": "iterations/s",
        "n_gpus": world,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": dt_max * 1e3 / steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"{'C3' if (m, n) == (4096, 8192) else ('C2' if (m, n) == (512, 1024) else 'custom')}: random dense planted LP m={m} n={n} fp64, one independent LP per GPU "
                               f"(seed = rank), reference default options, A resident in HBM",
                   "m": m, "n": n, "iterations_per_solve": iters_local / steps},
        "roofline": roofline,
    }
    if err is not None:
        out["config"]["max_abs_err_vs_planted_optimum"] = err
    if phase is not None:
        out["phase_ms_per_iteration"] = {k: v / phase_iters for k, v in phase.items()}
    if unbracketed is not None:
        out["unbracketed"] = unbracketed
    if want_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(A, b, c, m, n)
    return out, outputs


def measure_c4(steps, warmup, full, rank, local_rank, world, dist, dev, np, torch, lp_amd, synth):
    """BASELINE config 4: 32 independent 1024x2048 LPs per GPU (256 over 8), solved as ONE lockstep batch with the inputs
    resident in HBM; every x / tau goes device to device into the rank's packed block and ONE all-gather (RCCL) of those
    blocks ends the step.  value = LPs of all ranks / max-over-ranks wall time.  The members are the seeds of the
    committed oracle fixture (tests/golden/c4_members.npz): with `full`, after the timed region every member of this rank
    is compared with the oracle's OWN ENVELOPE on that LP (component-wise [min, max] of the oracle's x over its run on the
    LP as generated and four runs with permuted columns) widened by 1e-6, and its iteration count with the counts the
    oracle produced.  Returns (result dict for rank 0, number of members of ANY rank that fail that check (0 without
    `full`), the outputs of the last timed step)."""
    per_rank, m, n = 32, 1024, 2048
    seeds = [rank * per_rank + s for s in range(per_rank)]
    probs = [synth.planted_lp(s, m, n) for s in seeds]
    ctx = lp_amd.Context(local_rank)
    ctx.upload_lockstep([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs])   # untimed H2D
    opts = lp_amd.InteriorPoint.default().opts()
    xs = torch.zeros((per_rank, n), dtype=torch.float64, device=dev)
    gathered = torch.zeros((world * per_rank, n), dtype=torch.float64, device=dev) if dist is not None else None
    torch.cuda.synchronize()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def one_step():
        res = ctx.solve_lockstep_device(opts, xs.data_ptr(), n)    # returns when the rows are in place
        if any(r[0] != 0 for r in res):
            raise RuntimeError("a member of the shard did not solve")
        if dist is not None:                              # the single RCCL gather of the batch's solutions
            dist.all_gather_into_tensor(gathered, xs)
        return res

    for _ in range(warmup):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = one_step()
    barrier()
    dt = time.perf_counter() - t0
    its = sum(r[2] for r in res)
    x_host = xs.cpu().numpy()
    outputs = {"x": gathered.cpu().numpy() if dist is not None else x_host,
               "fun": [np.nan if r[1] is None else r[1] for r in res],
               "iterations": [r[2] for r in res], "status": [r[0] for r in res]}
    err = phase = parity = None
    nbad = 0
    if full:
        err = max(float(np.abs(x_host[k] - p[3]).max()) for k, p in enumerate(probs))
        # per-phase device times of one more lockstep solve (HIP events on the solver's stream), outside the timed region
        ctx.set_profiling(1)
        ctx.solve_lockstep_device(opts, xs.data_ptr(), n)
        pt = ctx.phase_times()
        ctx.set_profiling(0)
        batch_its = max(int(pt["iterations"]), 1)
        phase = {k: pt[k] / batch_its for k in ("adat_ms", "potrf_ms", "trsv_ms", "gemv_ms", "vec_ms", "total_ms")}
        parity, nbad = c4_parity(x_host, res, seeds, m, n, np)
    if dist is not None:
        t = torch.tensor([dt, float(nbad)], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt, nbad_any = float(t[0]), int(t[1])
    else:
        nbad_any = nbad
    ctx.close()
    lps = world * per_rank * steps / dt
    it_per_lp = its / per_rank
    # whole-solve MFMA fraction: the flops the path HAS to do in matrix form (A.D.A^T lower triangle + Cholesky) per LP-iteration
    flop_it = float(m) * (m + 1) * n + float(m) ** 3 / 3.0
    whole = lps / world * it_per_lp * flop_it / 1e12
    out = {
        "metric": "independent LPs solved per second, batch of 1024x2048 fp64 LPs sharded 32 per GPU", "value": lps,
        "unit": "LP/s", "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": dt * 1e3 / steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"C4: {world * per_rank} independent planted LPs m={m} n={n} fp64, {per_rank} per GPU as one lockstep batch, "
                               "inputs resident in HBM, solutions device to device into the packed block, one all-gather",
                   "iterations_per_lp": it_per_lp},
        "roofline": {"kernel": "whole solve of the shard (A.D.A^T + Cholesky flops of every LP-iteration / wall time per GPU)",
                     "bound": "mfma", "achieved": whole, "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s",
                     "frac": whole / PEAK_FP64_MFMA_TFLOPS, "traffic": None}}
    if full:
        adat_tf = per_rank * float(m) * (m + 1) * n / (phase["adat_ms"] * 1e-3) / 1e12 if phase["adat_ms"] > 0 else 0.0
        out["config"]["max_abs_err_vs_planted_optimum"] = err
        out["roofline"]["kernel"] += ("; adat_* = the batched A.D.A^T launch alone (32 LPs per launch, HIP events on the "
                                      "solver's stream)")
        out["roofline"].update(adat_achieved=adat_tf, adat_frac=adat_tf / PEAK_FP64_MFMA_TFLOPS, adat_launch_ms=phase["adat_ms"])
        out["phase_ms_per_lockstep_iteration"] = phase
        out["parity_rank0"] = parity
        out["parity_failed_members_any_rank"] = nbad_any
    return out, nbad_any, outputs


def c4_parity(x_host, res, seeds, m, n, np):
    """The members of this rank against the committed oracle fixture (measure_c4).  -> (parity record, failing members)."""
    parity = {"checked": False}
    gold = os.path.join(ROOT, "tests", "golden", "c4_members.npz")
    nbad = 0
    if os.path.exists(gold):
        g = np.load(gold)
        if int(g["m"]) == m and int(g["n"]) == n and max(seeds) < len(g["seeds"]) and "env_dlo" in g.files:
            e = np.array([np.abs(x_host[k] - g["x_slack"][s]).max() for k, s in enumerate(seeds)])
            lo = g["x_slack"][seeds] - g["env_dlo"][seeds].astype(np.float64)
            hi = g["x_slack"][seeds] + g["env_dhi"][seeds].astype(np.float64)
            excess = np.maximum(np.maximum(lo - x_host, x_host - hi), 0.0).max(axis=1)
            count_ok = np.array([res[k][2] in set(int(v) for v in g["iterations_all"][s]) for k, s in enumerate(seeds)])
            other_count = [int(s) for k, s in enumerate(seeds) if res[k][2] != int(g["iterations"][s])]
            width = (g["env_dlo"][seeds].astype(np.float64) + g["env_dhi"][seeds].astype(np.float64)).max(axis=1)
            # outside envelope + 1e-6: "parity unpinned" where the oracle's own runs span more than 1e-6 (reported, and a
            # failure only beyond one more envelope width); a count the oracle never produced is always a failure
            unpinned = [(int(s), float(excess[k]), float(width[k])) for k, s in enumerate(seeds) if excess[k] > 1e-6]
            bad = [(int(s), float(excess[k]), bool(count_ok[k])) for k, s in enumerate(seeds)
                   if excess[k] > max(1e-6, width[k]) or not count_ok[k]]
            nbad = len(bad)
            parity = {"checked": True, "members": len(seeds),
                      "tolerance": "every member: x inside the oracle's own envelope on that LP (5 oracle runs) widened by 1e-6, "
                                   "and an iteration count the oracle produced",
                      "max_abs_err_vs_oracle_run0": float(e.max()), "median_abs_err_vs_oracle_run0": float(np.median(e)),
                      "members_further_than_1e-6_from_oracle_run0": [int(s) for k, s in enumerate(seeds) if e[k] > 1e-6],
                      "members_with_another_count_than_oracle_run0": other_count,
                      "largest_excess_over_oracle_envelope": float(excess.max()),
                      "members_outside_envelope_plus_1e-6_parity_unpinned": unpinned,
                      "failed_members": bad}
    return parity, nbad


def bench_c4(args, rank, local_rank, world, dist, dev, np, torch, lp_amd, synth):
    out, nbad, outputs = measure_c4(args.steps, args.warmup, args.full, rank, local_rank, world, dist, dev, np, torch, lp_amd,
                                    synth)
    if rank == 0:
        dump_outputs(args.dump_outputs, outputs, np)
        emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if nbad:      # reduced over ranks: every rank (rank 0 included) exits non-zero when any member anywhere failed
        sys.stderr.write(f"bench c4: rank {rank}: {nbad} member(s) of some rank outside the parity tolerance: {out['parity_rank0']}\n")
        sys.exit(1)


if __name__ == "__main__":
    main()
