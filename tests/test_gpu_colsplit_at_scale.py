"""One LP split by columns over ranks (lpipm_set_collective + lpipm_upload_nsplit, lp_amd/colsplit.py) at the sizes where
its branches run: ONE iteration per rank count and shape against the oracle envelope, whole solves with every exit and
option on 2+ ranks, the raw ABI call and the state a context keeps between uploads.  All ranks are gloo processes that
share device 0 (as in test_gpu_colsplit.py): nothing here measures more than one GPU.

Which branch each shape reaches (host rules of upload_impl / plan_adat / enqueue_head: mp = m rounded up to 128, tile rows
T = mp / 128, column groups of M of POTRF_OUTER = 4 tile columns, G = ceil(T / 4); columns dealt to the ranks in whole
groups of 128, colsplit.column_range; per rank nblk = min(512, ceil(max(m, n_local) / 256))):

  world  m x n           mp    T   groups of M     columns per rank                what it adds
  2      1100 x 2300     1152  9   4, 4, 1         1152 / 1148                     short last group, 52 padding rows
  3      2049 x 4200     2176  17  4, 4, 4, 4, 1   1408 / 1408 / 1384              last group of one; 1024-wide super-blocks
  4      640 x 5000      640   5   4, 1            1280 x 3, 1160                  two groups, four ranks
  8      300 x 1100      384   3   3               256, 128 x 6, 76                9 column groups of A over 8 ranks
  5      130 x 700       256   2   2               256, 128, 128, 128, 60          world does not divide the 6 groups of A
  2      64 x 270000     128   1   1               135040 / 134960                 nblk = 512 on each rank: a thread's second
                                                                                   element feeds the cross-rank folds
  2      4096 x 8192     4096  32  4 x 8           4096 / 4096                     the C3 shape, one iteration
  2      300 x 900       384   3   3               512 / 388                       options: ip, tol, alpha0, the two QR arms
  2 | 3  150 x 512       256   2   2               256 / 256 | 256 / 128 / 128     exits: Infeasible, Unbounded, IterationLimit
  2 | 3  201 x 520       256   2   2               384 / 136 | 256 / 256 / 8       NumericalProblem: zero pivot in block 2
  2 | 3  301 x 1100      384   3   3               640 / 460 | 384 / 384 / 332     NumericalProblem: zero pivot in block 3
  3      256 x 1100      256   2   2               384 / 384 / 332                 18 .. 23 iterations (spread scenarios)
  2      1536 x 3072     1536  12  4, 4, 4         1536 / 1536                     on-stream contract with three groups

Collective accounting (derived from enqueue_residuals, enqueue_head, enqueue_tail, vec_final_x in solver.hip / kernels_vec.hip,
not from a run).  enqueue_residuals: A.x (m doubles) and the four scalars |r_D|^2, c.x, x.z, c.(x/tau) = 2 calls.
enqueue_head: one call per column group of M, mp (mp + 128) / 2 doubles in all (one call of that size when the context
reduces M in one block).  enqueue_tail: A.W (2 mp), {c.p, c.u, NaN flag} (3), the two minima (2), A.W (mp), c.u (1), the two
minima (2), then enqueue_residuals = 8 calls.  vec_final_x: 1 call of 1 double, only when x is returned.  So a solve that
ends after `it` iterations makes

    calls = 2 + it (G + 8) + (1 if x is returned)
    bytes = 8 [(m + 4) + it (mp (mp + 128) / 2 + 3 mp + m + 12) + (1 if x is returned)]

and one lpipm_k_iteration 2 + G + 8 calls.  Asserted as equalities on every rank.

Bounds.  One iteration: vector_checks.check_iteration with the project's fixed = 1e-8 and K = 4 around oracle.iteration,
the spread taken from the oracle on the column-permuted LP (as test_gpu_vector_stage_at_scale.py).  Whole solves: the
status and iteration count of oracle.solve and of the single-context solve, |x - x_oracle| <= 1e-6, |x - x_single| <= 1e-6,
fun to 1e-6 relative, log rows and fun bit-identical across ranks.

Inputs the oracle agrees with itself on.  "The oracle's iteration count" is a fair demand only where a column permutation
of the LP does not change the oracle's own count.  Every LP of the whole-solve tests was screened with the committed oracle
on the LP as generated and on two column permutations (status, iteration counts, max |x - x'|):

  planted seed 41, 130 x 700                       Optimal, 6 / 6 / 6, 2.7e-12
  planted seed 42, 300 x 1100                      Optimal, 6 / 6 / 6, 2.4e-11
  planted seed 43, 640 x 5000                      Optimal, 6 / 6 / 6, 3.8e-9
  planted seed 44, 1100 x 2300                     Optimal, 6 / 6 / 6, 1.9e-10
  planted seed 46, 2049 x 4200                     Optimal, 6 / 6 / 6, 5.4e-11
  planted seed 31, 300 x 900, ip = 0 | tol = 1e-6 | solver_type 1 | 2     Optimal, 6 / 6 / 6 each, <= 2.4e-8
  planted seed 32, 300 x 900, alpha0 = 0.9         Optimal, 10 / 10 / 10, 2.9e-12   (seed 31: 10 / 10 / 11, not used)
  |A|, -|b| of planted seed 21, 150 x 512          Infeasible, 5 / 5 / 5
  [B, -B], B = planted seed 22, 150 x 256, b = B u, u = 1 + default_rng(0).random(256), c = -1    Unbounded, 6 / 6 / 6
  planted seed 23, 150 x 512, max_iter = 5         IterationLimit, x within 6.1e-11
  planted seed 24, 200 x 520 + a zero row; seed 25, 300 x 1100 + a zero row    NumericalProblem at iteration 1 / 1 / 1
  spread_scenarios(seed, 256, 1100, [1.5])[0], seeds 53 | 54 | 55 | 59 | 61    Optimal, 18 | 19 | 19 | 18 | 18 on FIVE orders, <= 9e-9
  spread_scenarios(64, 256, 1100, [2.0])[0]        Optimal, 23 on five orders, 5.1e-8
  (not used: planted seed 45 1536 x 3072 pins x to 7.6e-6 only; s = 1.5 seed 56 gives 19 / 19 / 20; s = 2.0 seed 53 gives
   8.4e-7, seeds 57 .. 61 and 63 1.1e-6 .. 3e-6: too near the 1e-6 bound or past it)

The rank harness.  The cases are jobs (plain dicts: an LP recipe, options, what to call); the jobs of one rank count run
in ONE set of rank processes, started when the first test that needs them asks, because starting 2 .. 8 processes that
each load the GPU runtime costs more than most jobs.  Each rank reports each job through a queue as it finishes it; the
parent waits for every job with a time limit of the job's own (and every solve is capped at 60 iterations, so a solve
that does not converge costs seconds).  On a time limit, a reported exception, a missing result or
a non-zero exit code it terminates the ranks, and every test whose job has no result fails with that reason: nothing is
started again.  The process group has a two-minute timeout, so a rank that left the protocol fails the others instead
of parking them.  At most 8 ranks (8 rank processes + pytest with the GPU open); ranks are processes, never threads of
one process: each opens three streams (solver, look-ahead, communication) inside its own 4 hardware queues.
The time-out path of the group-wait kernel is not tested: it cannot be reached without making a launch hang.
"""
import ctypes as C
import functools
import os
import queue
import sys
import time
import traceback

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

OK, NUMERICAL_PROBLEM, INFEASIBLE, UNBOUNDED, ITERATION_LIMIT = 0, 2, 5, 6, 7
GLOO_TIMEOUT_S = 120             # init_process_group(timeout=): a collective whose peer never comes fails after this
START_LIMIT_S = 180              # rank processes up, GPU runtime loaded, process group formed
JOB_LIMIT_S = 60                 # one job on every rank (they take 0.1 .. 3 s); the jobs that say `limit=` get more
MAX_ITER = 60                    # every solve here, the oracle's and the single-context one too: the screened LPs need at most
                                 # 23 iterations, and a solve that a bug keeps from converging ends after 60, not after 1000
DEFAULT_MAX_ITER = 1000          # lpipm_default_opts; the 130 x 700 solve on 5 ranks runs with it (small enough to afford 1000)
MAX_RANKS = 8
REPLICATED = ("y", "d_y", "tau", "kappa", "d_tau", "d_kappa", "alpha", "info")


# ---------------------------------------------------------------------------------------------------------------------
# LPs and iterates by recipe: a small tuple that the parent and every rank turn into the same arrays
@functools.lru_cache(maxsize=3)
def _lp(recipe):
    from lp_amd import synth
    kind = recipe[0]
    if kind == "planted":
        return synth.planted_lp(*recipe[1:])[:3]
    if kind == "infeasible":                             # A >= 0, b <= 0, x >= 0: no solution
        A, b, c = synth.planted_lp(*recipe[1:])[:3]
        return np.abs(A), -np.abs(b), c
    if kind == "unbounded":                              # [B, -B] (u + t v, t v) is feasible for every t >= 0, v >= 0
        _, seed, m, nb = recipe
        B = synth.planted_lp(seed, m, nb)[0]
        u = 1.0 + np.random.default_rng(0).random(nb)
        return np.hstack([B, -B]), B @ u, -np.ones(2 * nb)
    if kind == "zero_row":                               # an all-zero last row: an exactly zero pivot of M
        A, b, c = synth.planted_lp(*recipe[1:])[:3]
        return np.vstack([A, np.zeros((1, A.shape[1]))]), np.concatenate([b, [0.0]]), c
    if kind == "spread":
        _, seed, m, n, s = recipe
        A, bs, cs, _ = synth.spread_scenarios(seed, m, n, [s])
        return A, bs[0], cs[0]
    if kind == "ratio":                                  # _ratio_recipe: the planted LP with c scaled and two columns swapped
        _, seed, m, n, sc, j, k = recipe
        A, b, c = synth.planted_lp(seed, m, n)[:3]
        P = np.arange(n)
        P[[j, k]] = P[[k, j]]
        return np.ascontiguousarray(A[:, P]), b, (sc * c)[P]
    raise ValueError(recipe)


def _iterate(spec, m, n):
    """("random", seed): as _iterate of test_gpu_vector_stage_at_scale.py with spread 1.5; ("flat", tau, kappa): x = z = 10,
    y = 0 (the ratio-test cases)."""
    if spec[0] == "flat":
        return np.full(n, 10.0), np.zeros(m), np.full(n, 10.0), float(spec[1]), float(spec[2])
    rng = np.random.default_rng(spec[1])
    x = np.exp(rng.uniform(-1.5, 1.5, n)); z = np.exp(rng.uniform(-1.5, 1.5, n))
    return x, rng.standard_normal(m), z, float(np.exp(rng.uniform(-1, 1))), float(np.exp(rng.uniform(-1, 1)))


def _opts(lp_amd, kw):
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in _capped(kw).items():
        setattr(o, k, v)
    return o


def _capped(kw):
    return {"max_iter": MAX_ITER, **kw}


# ---------------------------------------------------------------------------------------------------------------------
# what a rank does for one job
def _split(cx, rank, world, A, b, c, on_stream=None, raw=False):
    """set_collective + this rank's column block onto the context -> (collective, first column).  raw: the ABI's natural
    call, the block passed where it lies inside the row-major A (A + lo, lda = n_total), no copy."""
    from lp_amd import _capi
    from lp_amd.colsplit import TorchCollective, check_split, column_range
    m, n = A.shape
    check_split(n, world)
    cols = column_range(n, world, rank)
    coll = TorchCollective(cx.device, None, on_stream=on_stream)
    cx.set_collective(rank, world, coll)
    dp = C.POINTER(C.c_double)
    if raw:
        assert A.flags.c_contiguous and A.dtype == np.float64
        blk = A[:, cols.start:cols.stop]                 # a view: its data pointer is A + lo, its row stride n
        assert blk.ctypes.data == A.ctypes.data + 8 * cols.start and blk.strides == (8 * n, 8)
        cl, bb = np.ascontiguousarray(c[cols.start:cols.stop]), np.ascontiguousarray(b)
        rc = _capi.lib().lpipm_upload_nsplit(cx._h, m, n, len(cols), blk.ctypes.data_as(dp), n, bb.ctypes.data_as(dp),
                                             cl.ctypes.data_as(dp), 0.0)
        assert rc == 0, rc
        cx.m, cx.n = m, len(cols)
    else:
        cx.upload_column_block(np.ascontiguousarray(A[:, cols.start:cols.stop]), b, c[cols.start:cols.stop], n)
    return coll, cols.start


def _solve(cx, coll, opts, lo=0):
    c0, b0 = (coll.calls, coll.bytes) if coll is not None else (0, 0)
    rc, x, fun, it, rows = cx.solve_raw(opts, want_log=True)
    if coll is not None and coll.error is not None:
        raise coll.error
    return dict(rc=int(rc), lo=lo, x=x, fun=fun, it=int(it), rows=rows,
                calls=coll.calls - c0 if coll is not None else 0, bytes=coll.bytes - b0 if coll is not None else 0)


def _split_solve(lp_amd, rank, world, recipe, optkw, cx=None, **kw):
    own = cx is None
    cx = cx or lp_amd.Context(0)
    coll, lo = _split(cx, rank, world, *_lp(recipe), **kw)
    out = _solve(cx, coll, _opts(lp_amd, optkw), lo)
    if own:
        cx.close()
    return out


def _do(job, rank, world):
    import lp_amd
    kind = job["kind"]
    if kind == "solve":
        return _split_solve(lp_amd, rank, world, job["recipe"], job.get("opts", {}), on_stream=job.get("on_stream"))
    if kind == "iteration":
        A, b, c = _lp(job["recipe"])
        m, n = A.shape
        cx = lp_amd.Context(0)
        coll, lo = _split(cx, rank, world, A, b, c)
        x, y, z, tau, kappa = _iterate(job["iterate"], m, n)
        hi = lo + cx.n
        out = cx.k_iteration(_opts(lp_amd, {}), x[lo:hi], y, z[lo:hi], tau, kappa, ip=job["ip"])
        if coll.error is not None:
            raise coll.error
        out.update(lo=lo, calls=coll.calls, bytes=coll.bytes)
        cx.close()
        return out
    if kind == "raw":                    # the contiguous copy, then A + lo with lda = n_total, each on a fresh context
        return [_split_solve(lp_amd, rank, world, job["recipe"], {}, raw=raw) for raw in (False, True)]
    if kind == "sequence":               # column-split solves of changing shape on ONE context, each against a fresh context
        cx = lp_amd.Context(0)
        out = [(_split_solve(lp_amd, rank, world, r, {}, cx=cx), _split_solve(lp_amd, rank, world, r, {})) for r in job["recipes"]]
        cx.close()
        return out
    if kind == "plain_after":            # plain and lockstep uploads on a context that keeps set_collective(rank, world > 1)
        cx = lp_amd.Context(0)
        first = _split_solve(lp_amd, rank, world, job["recipe"], {}, cx=cx)
        coll = cx._collective
        opts = _opts(lp_amd, {})
        plain = []
        for r in job["plain"]:
            A, b, c = _lp(r)
            cx.upload_arrays(A, b, c)
            kept = _solve(cx, coll, opts)
            fresh = lp_amd.Context(0)
            fresh.upload_arrays(A, b, c)
            plain.append((kept, _solve(fresh, None, opts)))
            fresh.close()
        members = [_lp(r) for r in job["lockstep"]]
        calls0 = coll.calls
        cx.upload_lockstep([p[0] for p in members], [p[1] for p in members], [p[2] for p in members])
        lock_kept = cx.solve_lockstep(opts)
        fresh = lp_amd.Context(0)
        fresh.upload_lockstep([p[0] for p in members], [p[1] for p in members], [p[2] for p in members])
        lock_fresh = fresh.solve_lockstep(opts)
        fresh.close()
        cx.close()
        return dict(first=first, plain=plain, lock_kept=lock_kept, lock_fresh=lock_fresh, lock_calls=coll.calls - calls0)
    if kind == "two_ways":               # M reduced group by group behind the launch (default), then in one block after it
        out = []
        for env in (None, "0"):
            if env is not None:
                os.environ["LPIPM_EXPERIMENTAL"] = "1"          # knobs are read only with the master switch on
                os.environ["LPIPM_ADAT_UNITS"] = env
            cx = lp_amd.Context(0)
            os.environ.pop("LPIPM_ADAT_UNITS", None)
            os.environ.pop("LPIPM_EXPERIMENTAL", None)
            out.append(_split_solve(lp_amd, rank, world, job["recipe"], {}, cx=cx))
            cx.close()
        return out
    raise ValueError(kind)


def _worker(rank, world, port, q, jobs):
    """One rank: every job in order, each result (or the exception that ended this rank) reported as it happens."""
    name = None
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        import datetime
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=GLOO_TIMEOUT_S))
        q.put((rank, None, "ready", None))
        for job in jobs:
            name = job["name"]
            q.put((rank, name, "ok", _do(job, rank, world)))
        name = "the final barrier"
        dist.barrier()
        dist.destroy_process_group()
    except BaseException:                                # reported, not raised: the parent ends the other ranks
        q.put((rank, name, "error", traceback.format_exc()))


def _run(world, jobs):
    """-> {job name: [result of rank 0, 1, ...]} for the jobs every rank finished, {job name: reason (a str)} for the rest."""
    import torch.multiprocessing as mp
    assert 2 <= world <= MAX_RANKS
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = 29500 + (os.getpid() * 7 + world * 131 + int(time.time())) % 2000
    procs = [mpc.Process(target=_worker, args=(r, world, port, q, jobs)) for r in range(world)]
    for p in procs:
        p.start()
    results, failure = {}, None
    inbox = {}                   # (job name, rank) -> payload: the ranks' messages are not ordered against each other, so a
                                 # rank's next result may arrive before a slower peer's current one, and is kept here
    known = {None} | {job["name"] for job in jobs}
    seen = set()

    def collect(name, limit):
        """one message of every rank about `name` within `limit` seconds -> per-rank payloads, or the reason as a str"""
        deadline = time.monotonic() + limit
        while any((name, r) not in inbox for r in range(world)):
            try:
                rank, nm, tag, out = q.get(timeout=1.0)
            except queue.Empty:
                bad = [(i, p.exitcode) for i, p in enumerate(procs) if p.exitcode is not None and (name, i) not in inbox]
                if bad:
                    return f"rank processes ended without a result for {name or 'start-up'} (rank, exit code): {bad}"
                if time.monotonic() > deadline:
                    have = sorted(r for r in range(world) if (name, r) in inbox)
                    return f"time limit of {limit} s for {name or 'start-up'}: results of ranks {have} of {world} only"
                continue
            if tag == "error":
                return f"rank {rank} of {world} failed in {nm}:\n{out}"
            if nm not in known or (nm, rank) in seen:
                return f"rank {rank} reported {nm}, which is unknown or was reported before"
            inbox[(nm, rank)] = out
            seen.add((nm, rank))
        return [inbox.pop((name, r)) for r in range(world)]

    try:
        failure = collect(None, START_LIMIT_S)
        failure = failure if isinstance(failure, str) else None
        for job in jobs:
            if failure is not None:
                break
            got = collect(job["name"], job.get("limit", JOB_LIMIT_S))
            if isinstance(got, str):
                failure = got
            else:
                results[job["name"]] = got
        if failure is None:
            for i, p in enumerate(procs):
                p.join(timeout=GLOO_TIMEOUT_S + 30)
                if p.exitcode != 0:
                    failure = f"rank {i} of {world} ended with exit code {p.exitcode} after its last job"
                    results = {}
                    break
    finally:                                             # nothing is left running, whatever happened
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    for job in jobs:
        results.setdefault(job["name"], f"no result: {failure}")
    return results


# ---------------------------------------------------------------------------------------------------------------------
# the jobs, by rank count
ITER_CASES = [(2, 1100, 2300, 44), (3, 2049, 4200, 46), (4, 640, 5000, 43), (8, 300, 1100, 42), (5, 130, 700, 41),
              (2, 64, 270000, 6)]                       # (world, m, n, seed): ip False and True
ITER_C3 = (2, 4096, 8192, 7)                             # ip False only
SOLVE_CASES = ITER_CASES[:5]
OPTION_CASES = {"ip0": (31, dict(ip=0)), "tol1e-6": (31, dict(tol=1e-6)), "alpha0.9": (32, dict(alpha0=0.9)),
                "solver1": (31, dict(solver_type=1)), "solver2": (31, dict(solver_type=2))}
EXIT_CASES = {"infeasible": (("infeasible", 21, 150, 512), {}, INFEASIBLE),
              "unbounded": (("unbounded", 22, 150, 256), {}, UNBOUNDED),
              "iteration_limit": (("planted", 23, 150, 512), dict(max_iter=5), ITERATION_LIMIT),
              "zero_row_201": (("zero_row", 24, 200, 520), {}, NUMERICAL_PROBLEM),
              "zero_row_301": (("zero_row", 25, 300, 1100), {}, NUMERICAL_PROBLEM)}
SPREAD_CASES = [(53, 1.5), (54, 1.5), (55, 1.5), (59, 1.5), (61, 1.5), (64, 2.0)]
RATIO = dict(world=4, seed=43, m=640, n=5000,            # (scale of c, tau, kappa, the column that must block)
             x=(1.0, 1e-4, 1.0, 4999), z=(-1.0, 1e-4, 1.0, 2000), tau=(-1.0, 1.0, 1e-4, None))
SEQUENCE = [("planted", 42, 300, 1100), ("planted", 43, 640, 5000), ("planted", 42, 300, 1100)]
PLAIN_AFTER = dict(recipe=("planted", 42, 300, 1100), plain=[("planted", 47, 700, 1500), ("planted", 48, 1009, 1100)],
                   lockstep=[("planted", s, 256, 512) for s in (60, 61, 62)])


@functools.lru_cache(maxsize=None)
def _ratio_recipe(target):
    """-> (recipe, iterate spec) of the 640 x 5000 LP on 4 ranks whose step is limited by `target`: for x and z the column
    that limits the step of the planted LP (found by the oracle) is swapped into the place named in RATIO -- the last
    column (rank 3) for x, column 2000 (rank 1: 1280 .. 2559) for z."""
    from oracle import capi as oracle
    from test_gpu_vector_stage_at_scale import _blocker
    sc, tau, kappa, k = RATIO[target]
    seed, m, n = RATIO["seed"], RATIO["m"], RATIO["n"]
    it = ("flat", tau, kappa)
    A, b, c = _lp(("ratio", seed, m, n, sc, 0, 0))
    x, y, z, tau, kappa = _iterate(it, m, n)
    what, j = _blocker(oracle.iteration(A, b, c, x, y, z, tau, kappa), x, z, tau, kappa)
    assert what == target, (what, j)
    return ("ratio", seed, m, n, sc, j if k is not None else 0, k if k is not None else 0), it


def _jobs(world):
    jobs = []
    for w, m, n, seed in ITER_CASES + [ITER_C3]:
        if w == world:
            for ip in ((False, True) if (w, m, n, seed) != ITER_C3 else (False,)):
                jobs.append(dict(name=f"iteration {m}x{n} ip={int(ip)}", kind="iteration", recipe=("planted", seed, m, n),
                                 iterate=("random", 100 * seed + int(ip)), ip=ip, limit=150))
    for w, m, n, seed in SOLVE_CASES:
        if w == world:
            jobs.append(dict(name=f"solve {m}x{n}", kind="solve", recipe=("planted", seed, m, n), opts=_solve_kw(m), limit=150))
    if world == RATIO["world"]:
        for target in ("x", "z", "tau"):
            recipe, it = _ratio_recipe(target)
            jobs.append(dict(name=f"ratio {target}", kind="iteration", recipe=recipe, iterate=it, ip=False))
    if world == 2:
        for key, (seed, kw) in OPTION_CASES.items():
            jobs.append(dict(name=f"option {key}", kind="solve", recipe=("planted", seed, 300, 900), opts=kw))
        jobs.append(dict(name="raw", kind="raw", recipe=("planted", 42, 300, 1100)))
        jobs.append(dict(name="sequence", kind="sequence", recipes=SEQUENCE, limit=150))
        jobs.append(dict(name="plain_after", kind="plain_after", limit=150, **PLAIN_AFTER))
        for on in (False, True):
            jobs.append(dict(name=f"on_stream {int(on)}", kind="solve", recipe=("planted", 5, 1536, 3072), on_stream=on, limit=150))
    if world in (2, 3):
        for key, (recipe, kw, _) in EXIT_CASES.items():
            jobs.append(dict(name=f"exit {key}", kind="solve", recipe=recipe, opts=kw))
    if world == 3:
        for seed, s in SPREAD_CASES:
            jobs.append(dict(name=f"spread {seed} {s}", kind="solve", recipe=("spread", seed, 256, 1100, s)))
    if world in (2, 3):
        jobs.append(dict(name="two_ways", kind="two_ways", recipe=("planted", 44, 1100, 2300), limit=150))
    return jobs


def _solve_kw(m):
    return {"max_iter": DEFAULT_MAX_ITER} if m == 130 else {}


_GROUPS = {}


def _got(world, name):
    """The per-rank results of job `name`; the jobs of that rank count run once, when the first of them is asked for."""
    if world not in _GROUPS:
        t0 = time.monotonic()
        jobs = _jobs(world)
        _GROUPS[world] = _run(world, jobs)
        print(f"\n[measure] {world} ranks: {len(jobs)} jobs in {time.monotonic() - t0:.1f} s")
    res = _GROUPS[world][name]
    if isinstance(res, str):
        pytest.fail(f"{name} on {world} ranks: {res}")
    return res


# ---------------------------------------------------------------------------------------------------------------------
# checks
def _groups_of_M(m):
    return -(-(-(-m // 128)) // 4)


def _expected_traffic(m, it, with_x, groups=None):
    """(calls, bytes) of a column-split solve of `it` iterations (the module docstring derives it)"""
    mp = -(-m // 128) * 128
    G = _groups_of_M(m) if groups is None else groups
    return (2 + it * (G + 8) + int(with_x),
            8 * ((m + 4) + it * (mp * (mp + 128) // 2 + 3 * mp + m + 12) + int(with_x)))


def _stitch(got, n, key="x"):
    out = np.full(n, np.nan)
    for r in got:
        out[r["lo"]:r["lo"] + len(r[key])] = r[key]
    assert not np.isnan(out).any()
    return out


def _same_bits(a, b, what):
    assert a["rc"] == b["rc"] and a["it"] == b["it"], (what, a["rc"], b["rc"], a["it"], b["it"])
    assert np.array_equal(a["x"], b["x"], equal_nan=True), (what, float(np.nanmax(np.abs(a["x"] - b["x"]))))
    assert (a["fun"] == b["fun"] or (np.isnan(a["fun"]) and np.isnan(b["fun"]))) and a["rows"] == b["rows"], what


def _check_iteration(got, A, b, c, iterate, ip, seed, what):
    """stitched x, z, d_x, d_z + the replicated rest of rank 0 against the oracle envelope; the hard equalities"""
    from oracle import vector_checks as vc
    m, n = A.shape
    x, y, z, tau, kappa = iterate
    ref, spread = vc.iteration_envelope(A, b, c, x, y, z, tau, kappa, ip=ip, seed=seed)
    dev = {k: got[0][k] for k in REPLICATED}
    for k in ("x", "z", "d_x", "d_z"):
        dev[k] = _stitch(got, n, k)
    for r in got[1:]:                                    # replicated outputs: the same bits on every rank
        for k in REPLICATED:
            assert np.array_equal(np.asarray(r[k]), np.asarray(got[0][k])), (what, k, r["lo"])
    traffic = _expected_traffic(m, 1, False)            # the residuals at the point + one iteration: 2 + G + 8 calls
    assert all((r["calls"], r["bytes"]) == traffic for r in got), ([(r["calls"], r["bytes"]) for r in got], traffic)
    ratios = vc.check_iteration(dev, ref, spread)       # fixed = 1e-8, K = 4
    print(f"\n[measure] {what} ip={int(ip)} on {len(got)} ranks: worst ratio {max(ratios.values()):.3g} "
          f"({max(ratios, key=ratios.get)}), alpha {dev['alpha']:.6g}")
    if ip:                                               # alpha = 1 and the clamp at 1 (feasible_point.rs:96-105), everywhere
        for r in got:
            assert r["alpha"] == 1.0 and r["x"].min() >= 1.0 and r["z"].min() >= 1.0 and r["tau"] >= 1.0 and r["kappa"] >= 1.0
    return dev, ref


def _check_solve(ctx, got, recipe, optkw, want_rc, what, single=True):
    """every rank against oracle.solve and the single-context solve of the same LP; exact collective traffic"""
    import lp_amd
    from oracle import capi as oracle
    A, b, c = _lp(recipe)
    m, n = A.shape
    ref = oracle.solve(A, b, c, 0.0, oracle.default_opts(**_capped(optkw)))
    assert ref["status"] == want_rc, (what, ref["status"])
    has_x = want_rc in (OK, ITERATION_LIMIT)
    calls, nbytes = _expected_traffic(m, ref["iterations"], has_x)
    for r in got:
        assert r["rc"] == want_rc and r["it"] == ref["iterations"], (what, r["lo"], r["rc"], r["it"], ref["iterations"])
        assert r["rows"] == got[0]["rows"], (what, r["lo"])                   # replicated scalars: the same bits
        assert (r["calls"], r["bytes"]) == (calls, nbytes), (what, r["lo"], r["calls"], calls, r["bytes"], nbytes)
        if has_x:
            assert r["fun"] == got[0]["fun"]
            assert abs(r["fun"] - ref["fun"]) <= 1e-6 * max(1.0, abs(ref["fun"])), (what, r["fun"], ref["fun"])
    if single:
        ctx.upload_arrays(A, b, c)
        rc1, x1, fun1, it1, _ = ctx.solve_raw(_opts(lp_amd, optkw))
        assert rc1 == want_rc, (what, rc1)
        assert it1 == ref["iterations"], (what, it1, ref["iterations"])   # (a zero row: an exactly zero pivot on one context too)
    if has_x:
        x = _stitch(got, n)
        e_ref = float(np.abs(x - ref["x_slack"]).max())
        e_one = float(np.abs(x - x1).max()) if single else 0.0
        print(f"\n[measure] {what} on {len(got)} ranks: {ref['iterations']} iterations, |x - x_oracle| {e_ref:.3g}, "
              f"|x - x_single| {e_one:.3g}, {calls} calls, {nbytes / 1e6:.3g} MB")
        assert e_ref <= 1e-6 and e_one <= 1e-6, (what, e_ref, e_one)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 3. one iteration per rank count and shape
@pytest.mark.parametrize("world,m,n,seed,ip", [(*case, ip) for case in ITER_CASES for ip in (False, True)] + [(*ITER_C3, False)])
def test_one_iteration_on_ranks_within_the_oracle_envelope(world, m, n, seed, ip):
    got = _got(world, f"iteration {m}x{n} ip={int(ip)}")
    A, b, c = _lp(("planted", seed, m, n))
    _, ref = _check_iteration(got, A, b, c, _iterate(("random", 100 * seed + int(ip)), m, n), ip, seed, f"{m}x{n}")
    if not ip:
        assert (ref["d_x"] < 0).any() and (ref["d_x"] > 0).any()
        assert ref["alpha"] < 0.99995                     # the ratio test decided the step


@pytest.mark.parametrize("target", ["x", "z", "tau"])
def test_ratio_test_blocked_on_another_rank(target):
    """640 x 5000 on 4 ranks: the step is limited by an x element of the LAST rank, by a z element of rank 1, by tau.  A
    rank that took its own minimum instead of the reduced one would step further than the others."""
    from test_gpu_vector_stage_at_scale import _blocker
    recipe, spec = _ratio_recipe(target)
    got = _got(RATIO["world"], f"ratio {target}")
    A, b, c = _lp(recipe)
    m, n = A.shape
    x, y, z, tau, kappa = _iterate(spec, m, n)
    dev, ref = _check_iteration(got, A, b, c, (x, y, z, tau, kappa), False, RATIO["seed"], f"blocked by {target}")
    k = RATIO[target][3]
    want = (target, k) if k is not None else (target, -1)
    assert _blocker(ref, x, z, tau, kappa) == want
    assert _blocker(dev, x, z, tau, kappa) == want
    if k is not None:                                    # the blocking element is not rank 0's
        owner = [i for i, r in enumerate(got) if r["lo"] <= k < r["lo"] + len(r["x"])]
        assert owner == [{"x": 3, "z": 1}[target]]
    assert dev["alpha"] < 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 4. whole solves, options and exits on 2+ ranks
@pytest.mark.parametrize("world,m,n,seed", SOLVE_CASES)
def test_solve_on_ranks_matches_oracle_and_single(ctx, world, m, n, seed):
    _check_solve(ctx, _got(world, f"solve {m}x{n}"), ("planted", seed, m, n), _solve_kw(m), OK, f"{m}x{n}")


@pytest.mark.parametrize("key", list(OPTION_CASES))
def test_options_on_two_ranks(ctx, key):
    """300 x 900 on 2 ranks (512 / 388 columns): ip off, a looser tol, a shorter alpha0, and the two QR arms against the
    oracle's same arm."""
    seed, kw = OPTION_CASES[key]
    ref = _check_solve(ctx, _got(2, f"option {key}"), ("planted", seed, 300, 900), kw, OK, f"300x900 {key}")
    if key == "alpha0.9":
        assert ref["iterations"] >= 10                   # the option reached the step length


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("key", list(EXIT_CASES))
def test_exits_agree_on_all_ranks(ctx, world, key):
    """Infeasible, Unbounded, IterationLimit (x is returned) and NumericalProblem (a zero pivot of the replicated factor) with
    2 and 3 ranks: the status and the iteration count of the oracle on every rank.  Ranks that decided differently would
    leave each other in a collective: the harness would end them and fail the test."""
    recipe, kw, want = EXIT_CASES[key]
    got = _got(world, f"exit {key}")
    if key == "zero_row_201" and world == 3:
        assert [len(r["x"]) for r in got] == [256, 256, 8]                     # the smallest block there is
    _check_solve(ctx, got, recipe, kw, want, f"{key}")


@pytest.mark.parametrize("seed,s", SPREAD_CASES)
def test_long_trajectories_on_three_ranks(ctx, seed, s):
    """256 x 1100 spread scenarios on 3 ranks (384 / 384 / 332 columns): 18 .. 23 iterations instead of the planted LPs' 6."""
    ref = _check_solve(ctx, _got(3, f"spread {seed} {s}"), ("spread", seed, 256, 1100, s), {}, OK, f"spread s={s} seed {seed}")
    assert ref["iterations"] >= 18


# ---------------------------------------------------------------------------------------------------------------------
# 5. ABI and context state
def test_raw_abi_upload_with_lda_n_total():
    """lpipm_upload_nsplit(A + lo, lda = n_total) on 2 ranks at 300 x 1100: the same bits as the contiguous copy of the block."""
    for copy, raw in _got(2, "raw"):
        assert copy["rc"] == OK and copy["it"] == 6
        _same_bits(copy, raw, "raw")
        assert (copy["calls"], copy["bytes"]) == (raw["calls"], raw["bytes"])


def test_column_split_uploads_of_changing_shape_on_one_context():
    """300 x 1100, then 640 x 5000 (m changes: the packed buffer of M is reallocated), then 300 x 1100 again on one context
    per rank: each the same bits as on a fresh context."""
    for rank, steps in enumerate(_got(2, "sequence")):
        assert len(steps) == len(SEQUENCE)
        for i, (kept, fresh) in enumerate(steps):
            assert fresh["rc"] == OK
            _same_bits(kept, fresh, ("sequence", rank, i))
            assert (kept["calls"], kept["bytes"]) == (fresh["calls"], fresh["bytes"]) == \
                _expected_traffic(SEQUENCE[i][2], fresh["it"], True)


def test_plain_and_lockstep_uploads_on_a_context_that_keeps_its_collective():
    """set_collective(rank, 2) stays on the context after a column-split solve; plan_adat then gives every later single
    upload the units kernel.  At 700 x 1500 and 1009 x 1100 a fresh context takes the stream-K kernel (21 and 36 tiles,
    several chunks, under 256 units): units against stream-K must give the same bits, and the callback is not called."""
    from test_gpu_shared_matrix_at_scale import _plan
    for r in PLAIN_AFTER["plain"]:
        assert _plan(r[2], r[3])["single_streamk"], r
    for out in _got(2, "plain_after"):
        assert out["first"]["rc"] == OK
        for kept, fresh in out["plain"]:
            assert fresh["rc"] == OK and kept["calls"] == 0 and kept["bytes"] == 0
            _same_bits(kept, fresh, "plain upload after a column-split solve")
        assert out["lock_calls"] == 0 and len(out["lock_kept"]) == len(PLAIN_AFTER["lockstep"])
        for (st, x, f, it), (st0, x0, f0, it0) in zip(out["lock_kept"], out["lock_fresh"]):
            assert st == st0 == OK and it == it0 and np.array_equal(x, x0) and f == f0


@pytest.mark.parametrize("world", [2, 3])
def test_grouped_against_one_block_reduction_with_a_short_last_group(world):
    """1100 x 2300: groups of 4, 4 and 1 tile columns of M summed over the ranks one by one behind the running launch,
    against the whole packed triangle in one block after it: (G - 1) more calls per iteration, the same bytes, and both
    within 1e-6 of the oracle.
    Two ranks: the same bits, whatever the all-reduce does -- a sum of two terms has one value.  Three ranks: NOT the same
    bits with gloo, and no fault of the library: gloo's ring sums an element's three terms in an order that depends on
    where the element sits in the buffer, so reducing the same doubles as one block or as three slices differs in the last
    bit of about a sixth of them (reproduced with CPU tensors alone: 130223 of the 737280 doubles of this packed triangle,
    1.8e-15 apart).  Measured here on 3 ranks: x of the two ways 9.1e-11 apart, the same 6 iterations.  So on three ranks
    the two ways are held to the oracle, to the same status and iteration count and to 1e-9 of each other, each
    bit-identical across its ranks."""
    from oracle import capi as oracle
    G = _groups_of_M(1100)
    assert G == 3
    got = _got(world, "two_ways")
    A, b, c = _lp(("planted", 44, 1100, 2300))
    ref = oracle.solve(A, b, c, 0.0, oracle.default_opts(**_capped({})))
    for k, way in enumerate(("grouped", "one block")):
        x = _stitch([r[k] for r in got], 2300)
        assert all(r[k]["rc"] == OK == ref["status"] and r[k]["it"] == ref["iterations"] for r in got)
        assert all(r[k]["rows"] == got[0][k]["rows"] and r[k]["fun"] == got[0][k]["fun"] for r in got)
        err = float(np.abs(x - ref["x_slack"]).max())
        print(f"\n[measure] 1100x2300 on {world} ranks, M reduced {way}: |x - x_oracle| {err:.3g}")
        assert err <= 1e-6
    for grouped, block in got:
        if world == 2:
            _same_bits(grouped, block, "grouped / one block")
        assert grouped["calls"] == block["calls"] + (G - 1) * grouped["it"] and grouped["bytes"] == block["bytes"]
        assert (grouped["calls"], grouped["bytes"]) == _expected_traffic(1100, grouped["it"], True)
        assert (block["calls"], block["bytes"]) == _expected_traffic(1100, block["it"], True, groups=1)
    dx = float(np.abs(_stitch([r[0] for r in got], 2300) - _stitch([r[1] for r in got], 2300)).max())
    print(f"[measure] 1100x2300 on {world} ranks: |x_grouped - x_block| {dx:.3g}")
    # the two ways differ in the last bit of entries of M and in nothing else; the oracle, whose every sum changes under a
    # column permutation, moves x of this LP by 1.9e-10 (the header's screening): five times that, far inside the 1e-6
    assert dx <= 1e-9, dx


def test_on_stream_contract_with_three_groups():
    """lpipm_set_collective_on_stream(1) at 1536 x 3072 on 2 ranks: three groups of M go through the callback on the
    communication stream without a drain in front.  The same bits as the drained contract."""
    for drained, on in zip(_got(2, "on_stream 0"), _got(2, "on_stream 1")):
        assert drained["rc"] == OK
        _same_bits(drained, on, "on-stream")
        assert (drained["calls"], drained["bytes"]) == (on["calls"], on["bytes"]) == _expected_traffic(1536, on["it"], True)
