"""Records what the tail of an iteration computes in every form it takes.

iteration_tail_parent.json : per case a record of return code, status, iteration count and SHA-256 of the bytes of fun and x (of a
                             single LP also of its iteration log); of the kernel entries lpipm_k_iteration and
                             lpipm_k_tall_sym_solve the hashes of everything they return; of a profiled solve the integer fields
                             of its phase times.  Plus the CU count of the device it was recorded on (kernel plans, and with them
                             the bits of a solve, depend on it).  tests/test_gpu_iteration_tail.py replays every case on the code
                             under test and requires equality.

The shapes are those at which each branch of the tail is taken: m no multiple of 128, n past the fused vector stage's limit of
1024, the look-ahead at its forced threshold, a refining context, both QR arms, equality rows, every batch form and a column
split over two ranks.  tests/golden/solve_contract.json covers the entries' contract at tiny shapes, fused stage only.

The record is the behaviour of the commit it was taken at (the parent of the one that made the tail one sequence of named
steps): regenerate it only at a commit whose results are the intended ones, never to make a failing replay pass.  Only the public
Python API is used, so the script runs unchanged at any commit that has it.  The record is taken twice and written only if both
runs agree.
Run from the repo root on an MI355X:  python tests/golden/make_iteration_tail.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "iteration_tail_parent.json")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()[:32]


# ---------------------------------------------------------------- problems
def planted_eq(seed, m, nx, me):
    """tests/test_tall_eq_host.py's planted vertex of min c^T x, X x <= b, A_eq x = b_eq, x >= 0.  -> X, b, A_eq, b_eq, c"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    Ae = rng.standard_normal((me, nx))
    k = min(nx, max(nx // 2, me))
    na = max(k - me, 0)
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:na]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, na)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    c = -X.T @ lam + Ae.T @ rng.standard_normal(me) + mu
    return X, b, Ae, Ae @ xs, c


def tall_problem(seed, m, nx, me):
    import lp_amd
    X, b, Ae, be, c = planted_eq(seed, m, nx, me)
    p = lp_amd.Problem.target(c).ub(X, b)
    return (p.eq(Ae, be) if me else p).build()


def shared_vectors(seed, X, Ae, K):
    """K members (b, c) over the blocks X (`ub`) and Ae (`eq`, may have no rows), each with an interior primal and dual point."""
    rng = np.random.default_rng(seed)
    m, nx = X.shape
    bs, cs = [], []
    for _ in range(K):
        xs = rng.uniform(0.5, 1.5, nx)
        bs.append(np.concatenate([X @ xs + rng.uniform(0.5, 1.5, m), Ae @ xs]))
        cs.append(-X.T @ rng.uniform(0.5, 1.5, m) + Ae.T @ rng.standard_normal(Ae.shape[0]) + rng.uniform(0.5, 1.5, nx))
    return bs, cs


def dense_shared_vectors(seed, A, K):
    """K members (b, c) of min c^T x, A x = b, x >= 0 over one A, each with an interior primal and dual point."""
    rng = np.random.default_rng(seed)
    m, n = A.shape
    return ([A @ rng.uniform(0.5, 1.5, n) for _ in range(K)],
            [A.T @ rng.standard_normal(m) + rng.uniform(0.5, 1.5, n) for _ in range(K)])


def opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


# ---------------------------------------------------------------- records
def single(ctx, **kw):
    """[rc, status, iterations, sha(fun), sha(x), sha(log)] of one logged solve of what is resident (a single LP's status is its
    return code)."""
    rc, x, fun, it, rows = ctx.solve_raw(opts(**kw), want_log=True)
    return [int(rc), int(rc), int(it), _sha([fun]), _sha(x), _sha(np.array(rows, dtype=np.float64))]


def lockstep(ctx, **kw):
    """[rc, [status, iterations, sha(fun), sha(x) | null] per member] (a call that fails raises: rc is Ok)"""
    members = ctx.solve_lockstep(opts(**kw))
    return [0, [[int(st), int(it), _sha([np.nan if fun is None else fun]), None if x is None else _sha(x)]
                for st, x, fun, it in members]]


def iteration(ctx, seed):
    """lpipm_k_iteration from one seeded iterate with ip 0 and 1: hashes of everything it returns."""
    rng = np.random.default_rng(seed)
    x, z, y = rng.uniform(0.5, 2.0, ctx.n), rng.uniform(0.5, 2.0, ctx.n), rng.standard_normal(ctx.m)
    rec = {}
    for ip in (0, 1):
        r = ctx.k_iteration(opts(), x, y, z, 1.25, 0.75, ip=bool(ip))
        rec[f"ip{ip}"] = {k: (int(r[k]) if k == "info" else _sha(r[k] if isinstance(r[k], np.ndarray) else [r[k]]))
                          for k in ("x", "y", "z", "d_x", "d_y", "d_z", "tau", "kappa", "d_tau", "d_kappa", "alpha", "info")}
    return rec


def tall_sym_solve(ctx, seed):
    """lpipm_k_tall_sym_solve with 1 and 2 right-hand sides: hashes of U and V, and the pivot word."""
    rng = np.random.default_rng(seed)
    dinv = rng.uniform(0.5, 2.0, ctx.n)
    rec = {}
    for nrhs in (1, 2):
        U, V, info = ctx.k_tall_sym_solve(dinv, rng.standard_normal((nrhs, ctx.n)), rng.standard_normal((nrhs, ctx.m)))
        rec[f"nrhs{nrhs}"] = [_sha(U), _sha(V), int(info)]
    return rec


def profiled(ctx):
    """The integer fields of the phase times of one profiled solve (no times)."""
    ctx.set_profiling(1)
    rc = ctx.solve_raw(opts())[0]
    t = ctx.phase_times()
    ctx.set_profiling(0)
    return [int(rc)] + [int(t[k]) for k in ("iterations", "adat_launches", "gemv_passes")]


# ---------------------------------------------------------------- the column split
def _split_worker(rank, world, port, q, seed, m, n):
    """One rank of tests/test_gpu_colsplit.py's harness: gloo ranks that share cuda:0, each with a block of whole column groups."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from lp_amd import synth
    from lp_amd.colsplit import column_range, solve_column_split
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    A, b, c = synth.planted_lp(seed, m, n)[:3]
    cols = column_range(n, world, rank, 128)
    rc, x, fun, it, rows, _ = solve_column_split(np.ascontiguousarray(A[:, cols.start:cols.stop]), b, c[cols.start:cols.stop], n, 0.0,
                                                 opts(), want_log=True)
    q.put((rank, [int(rc), int(rc), int(it), _sha([fun]), _sha(x), _sha(np.array(rows, dtype=np.float64))]))
    dist.barrier()
    dist.destroy_process_group()


def column_split(seed, m, n, world=2):
    """-> one single-LP record per rank (x: the rank's slice)."""
    import torch.multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = 29500 + (os.getpid() * 7 + world * 131 + m + 1) % 2000
    procs = [mpc.Process(target=_split_worker, args=(r, world, port, q, seed, m, n)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [rec for _, rec in got]


# ---------------------------------------------------------------- the cases
class Knobs:
    """Environment knobs of the library for the duration of a block; setenv / delenv are the caller's (the test: monkeypatch's).
    A knob is read only with the master switch LPIPM_EXPERIMENTAL on; most are read when a context is created."""
    def __init__(self, setenv, delenv, **kw):
        self.setenv, self.delenv, self.kw = setenv, delenv, kw

    def __enter__(self):
        if self.kw:
            self.setenv("LPIPM_EXPERIMENTAL", "1")
        for k, v in self.kw.items():
            self.setenv(k, v)

    def __exit__(self, *exc):
        for k in list(self.kw) + (["LPIPM_EXPERIMENTAL"] if self.kw else []):
            self.delenv(k)


def cases(setenv, delenv):
    """-> {label: record}, every upload on a context of its own."""
    import lp_amd
    from lp_amd import synth
    rec = {}

    def on_context(upload, body, **knobs):
        with Knobs(setenv, delenv, **knobs):
            ctx = lp_amd.Context(0)
            try:
                upload(ctx)
                body(ctx)
            finally:
                ctx.close()

    A, b, c = synth.planted_lp(0, 200, 300)[:3]
    dense = lambda ctx: ctx.upload_arrays(A, b, c)
    A2, b2, c2 = synth.planted_lp(1, 130, 1300)[:3]
    dense_wide = lambda ctx: ctx.upload_arrays(A2, b2, c2)
    tall, tall_eq = tall_problem(2, 600, 40, 0), tall_problem(3, 600, 40, 5)
    up_tall = lambda ctx: ctx.upload(tall, tall=True)
    up_tall_eq = lambda ctx: ctx.upload_tall_eq(tall_eq)

    # ---- whole solves: every form of the tail
    def two_solves(ctx):                            # the second replays the kept first factor
        rec["dense:200x300:first"] = single(ctx)
        rec["dense:200x300:again"] = single(ctx)
    on_context(dense, two_solves)
    on_context(dense, lambda ctx: rec.__setitem__("dense:200x300:refine2", single(ctx)), LPIPM_REFINE="2")
    on_context(dense, lambda ctx: rec.__setitem__("dense:200x300:inverse", single(ctx, solver_type=int(lp_amd.EquationSolverType.Inverse))))
    on_context(dense, lambda ctx: rec.__setitem__("dense:200x300:least_squares", single(ctx, solver_type=int(lp_amd.EquationSolverType.LeastSquares))))
    on_context(dense, lambda ctx: rec.__setitem__("dense:200x300:unfused", single(ctx)), LPIPM_VEC_FUSED="0")
    on_context(dense_wide, lambda ctx: rec.__setitem__("dense:130x1300", single(ctx)))
    A3, b3, c3 = synth.planted_lp(0, 1536, 3072)[:3]
    on_context(lambda ctx: ctx.upload_arrays(A3, b3, c3), lambda ctx: rec.__setitem__("dense:1536x3072:lookahead1", single(ctx)),
               LPIPM_LOOKAHEAD="1")
    on_context(up_tall, lambda ctx: rec.__setitem__("tall:600x40", single(ctx)))
    on_context(up_tall_eq, lambda ctx: rec.__setitem__("tall_eq:600x40+5", single(ctx)))
    X, _, Ae, _, _ = planted_eq(3, 600, 40, 5)
    bs, cs = shared_vectors(4, X, Ae, 3)
    on_context(lambda ctx: ctx.upload_lockstep_shared_ub_eq_tall(X, Ae, bs, cs),
               lambda ctx: rec.__setitem__("shared_tall_eq:3x600x40+5", lockstep(ctx)))
    own = [planted_eq(10 + i, 600, 40, 0) for i in range(3)]
    on_context(lambda ctx: ctx.upload_lockstep_ub_tall([o[0] for o in own], [o[1] for o in own], [o[4] for o in own]),
               lambda ctx: rec.__setitem__("owned_tall:3x600x40", lockstep(ctx)))
    sb, sc = dense_shared_vectors(5, A, 3)
    on_context(lambda ctx: ctx.upload_lockstep_shared(A, sb, sc), lambda ctx: rec.__setitem__("shared:3x200x300", lockstep(ctx)))
    lock = [synth.planted_lp(20 + i, 130, 260)[:3] for i in range(16)]
    on_context(lambda ctx: ctx.upload_lockstep([l[0] for l in lock], [l[1] for l in lock], [l[2] for l in lock]),
               lambda ctx: rec.__setitem__("lockstep:16x130x260", lockstep(ctx)))        # two half-batch views
    rec["colsplit:2x256x512"] = column_split(0, 256, 512)

    # ---- one iteration from a seeded iterate; the reduced sym_solve alone
    for label, up in (("dense:200x300", dense), ("dense:130x1300", dense_wide), ("tall:600x40", up_tall), ("tall_eq:600x40+5", up_tall_eq)):
        on_context(up, lambda ctx: rec.__setitem__(f"k_iteration:{label}", iteration(ctx, 30)))
    for label, up in (("tall:600x40", up_tall), ("tall_eq:600x40+5", up_tall_eq)):
        on_context(up, lambda ctx: rec.__setitem__(f"k_tall_sym_solve:{label}", tall_sym_solve(ctx, 31)))

    # ---- more equality rows than columns: NumericalProblem
    over = tall_problem(6, 60, 4, 6)

    def overdetermined(ctx):
        rc, _, _, it, _ = ctx.solve_raw(opts())
        rec["tall_eq:60x4+6"] = [int(rc), int(it)]
    on_context(lambda ctx: ctx.upload_tall_eq(over), overdetermined)

    # ---- the counters of a profiled solve
    on_context(dense, lambda ctx: rec.__setitem__("profiled:dense:200x300", profiled(ctx)))
    on_context(up_tall_eq, lambda ctx: rec.__setitem__("profiled:tall_eq:600x40+5", profiled(ctx)))
    return rec


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def load(path=OUT):
    with open(path) as f:
        return json.load(f)


def main():
    setenv, delenv = os.environ.__setitem__, lambda k: os.environ.pop(k, None)
    first, second = cases(setenv, delenv), cases(setenv, delenv)
    differ = sorted(k for k in first if first[k] != second[k])
    assert not differ, f"two runs on one commit differ in {differ}: nothing written"
    doc = dict(note="recorded by tests/golden/make_iteration_tail.py; a solve is [rc, status, iterations, sha256(fun), sha256(x), "
                    "sha256(log)] (hashes cut to 32 hex digits), a batch [rc, [[status, iterations, sha256(fun), sha256(x)] per member]]",
               cu_count=cu_count(), cases=first)
    with open(OUT, "w") as f:
        f.write('{"note":%s,\n"cu_count":%d,\n"cases":{\n' % (json.dumps(doc["note"]), doc["cu_count"]))
        f.write(",\n".join("%s:%s" % (json.dumps(k), json.dumps(first[k], separators=(",", ":"))) for k in sorted(first)))
        f.write("\n}}\n")
    assert load() == json.loads(json.dumps(doc))
    print(len(first), "cases, CU count", doc["cu_count"], "taken twice, identical")
    for k in sorted(first):
        print(k, json.dumps(first[k])[:150])


if __name__ == "__main__":
    main()
