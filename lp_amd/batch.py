"""Batches of independent LPs sharded one-shard-per-GPU (BASELINE config C4 / SURVEY.md 8e).

LPs are independent, so the path shards with NO data-path collective: rank r solves the contiguous
block `shard_range(count, world, r)` on its own GPU (its own lpipm_ctx / stream), and the batch ends
with exactly ONE collective -- an all-gather (RCCL over xGMI when the backend is "nccl") of a packed
[shard_max, n_max + 3] DEVICE block per rank holding x / tau, fun, iterations and status of each LP.
On the GPU the shard goes to lpipm_solve_batch_device in one call: LPs of equal shape advance as lockstep
batches (one kernel launch covers all of them), odd shapes one at a time, and every member's x / tau is
copied device to device into its row of the packed block -- no solution vector visits the host before the
gather (only the 3 scalars per LP do).
One process per GPU, `torch.distributed` for the plumbing; nothing here computes on the CPU.
`solve_fn` exists so that the sharding / packing / gather logic can be unit-tested on CPU ranks
(gloo) with an injected solver; the default is the HIP path and it fails loudly without a GPU.
"""
from __future__ import annotations

import numpy as np

from . import has_x


def shard_range(count: int, world: int, rank: int) -> range:
    """Static block partition: the first `count % world` ranks get one extra LP."""
    base, extra = divmod(count, world)
    lo = rank * base + min(rank, extra)
    return range(lo, lo + base + (1 if rank < extra else 0))



def solve_batch_sharded(problems, opts=None, ctx=None, group=None, device=None, solve_fn=None, tall=False):
    """problems: sequence of (A, b, c, c0) or (A, b, c, c0, n_slack) -- every rank passes the same list (or at least its shard
    at the right indices).  Returns, on EVERY rank, a list of dicts {status, x_slack, fun, iterations}
    in problem order.  `solve_fn(A, b, c, c0, None) -> (status, x | None, fun, iterations)` replaces the
    library call in the CPU-rank tests.
    tall=True: problems are lp_amd.Problems built from `ub` rows only (else ValueError, before any device or rank is
    touched); each shard goes through Context.solve_batch_device(..., tall=True) and x_slack has n + m_ub entries."""
    import torch
    import torch.distributed as dist

    if tall:
        import lp_amd
        if solve_fn is not None:
            raise ValueError("tall=True runs the library call: it takes no solve_fn")
        A_ubs = lp_amd._tall_members(problems)[0]
        tall_problems = problems
        # the rest of this function only reads a member's length of x, from its c: n + m_ub entries in the tall form
        problems = [(None, None, np.broadcast_to(0.0, (A.shape[0] + A.shape[1],)), 0.0) for A in A_ubs]

    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    count = len(problems)
    mine = shard_range(count, world, rank)
    shard_max = -(-count // world) if count else 0
    n_max = max((np.asarray(p[2]).shape[0] for p in problems), default=0)
    rows = max(shard_max, 1)
    meta = np.zeros((rows, 3))
    meta[:, 2] = -1.0                                 # status -1: padding slot, no LP here
    if solve_fn is None:                              # the product path: the whole shard in one library call
        import lp_amd
        ctx = ctx or lp_amd.default_context(device.index if device is not None and device.index is not None else 0)
        opts = opts or lp_amd.InteriorPoint.default().opts()
        device = device or torch.device("cuda", ctx.device)
        packed = torch.zeros((rows, n_max + 3), dtype=torch.float64, device=device)
        torch.cuda.synchronize(device)                # the zero fill runs on torch's stream, the solver on its own
        if tall:
            res = ctx.solve_batch_device([tall_problems[i] for i in mine], opts, packed.data_ptr(), n_max + 3, tall=True)
        else:
            res = ctx.solve_batch_device([problems[i] for i in mine], opts, packed.data_ptr(), n_max + 3)
        for slot, (rc, fun, it) in enumerate(res):
            meta[slot] = (fun if fun is not None else float("nan"), float(it), float(rc))
        packed[:, n_max:] = torch.from_numpy(meta).to(device)       # 3 scalars per LP; x rows never left the device
    else:                                             # CPU-rank tests: injected solver, host rows
        device = device or torch.device("cpu")
        host = np.zeros((rows, n_max + 3))
        for slot, i in enumerate(mine):
            A, b, c, c0 = problems[i][:4]
            n = np.asarray(c).shape[0]
            rc, x, fun, it = solve_fn(A, b, c, c0, None)
            if x is not None:
                host[slot, :n] = np.asarray(x, dtype=np.float64)
            meta[slot] = (fun if has_x(rc) and fun is not None else float("nan"), float(it), float(rc))
        host[:, n_max:] = meta
        packed = torch.from_numpy(host).to(device)
    if world > 1:
        flat = torch.empty((world * packed.shape[0], packed.shape[1]), dtype=torch.float64, device=device)
        dist.all_gather_into_tensor(flat, packed, group=group)         # the single collective of the batch
        gathered = flat.view(world, packed.shape[0], packed.shape[1])
    else:
        gathered = packed.unsqueeze(0)
    g = gathered.cpu().numpy()
    out = []
    for i in range(count):
        r = next(rr for rr in range(world) if i in shard_range(count, world, rr))
        slot = i - shard_range(count, world, r).start
        row = g[r, slot]
        n = np.asarray(problems[i][2]).shape[0]
        status = int(row[n_max + 2])
        out.append(dict(status=status, x_slack=row[:n].copy() if has_x(status) else None,
                        fun=float(row[n_max]) if has_x(status) else None, iterations=int(row[n_max + 1])))
    return out


def solve_shared_matrix(A, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, n_slack=0, duals=False, certificates=False):
    """LPs that share ONE constraint matrix A (scenario sweeps: only b, c and c0 vary), member i = (A, bs[i], cs[i], c0s[i]).
    The members go through lockstep groups of at most `max_group` on one context (lpipm_upload_lockstep_shared: A resident
    once, every pass over it serving the whole group).  Returns a list of dicts {status, x_slack, fun, iterations} in member
    order, as solve_batch_sharded does.  n_slack: the last n_slack columns of A are its slack block [I; 0], kept structural
    (lpipm_upload_lockstep_shared_slack).
    duals=True (here and in every solve_shared_* / sweep_shared_* below): each member's dict gains y, z and dual_fun
    (Context.duals: None for a member without a solution), fetched after each group's solve_lockstep -- a scenario-cut loop
    reads its cuts from y.
    certificates=True (likewise): each member WITHOUT a solution gains cert_kind, cert_y, cert_col, cert_scale and
    cert_residual (Context.certificate's kind, y, col, scale, residual), fetched where duals=True fetches its rows -- the
    feasibility cut of an infeasible scenario is cert_y."""
    return _groups(lambda cx, b, c, c0: cx.upload_lockstep_shared(A, b, c, c0, n_slack=n_slack), bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def solve_shared_ub_eq(A_ub, A_eq, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, duals=False, certificates=False):
    """Inequality-form LPs over ONE pair of blocks (right-hand-side and cost sweeps over A_ub x <= b_ub, A_eq x == b_eq):
    member i = (bs[i] = [b_ub_i; b_eq_i], cs[i] = the n structural costs, c0s[i]); either block may be None.  Lockstep groups
    of at most `max_group` on one context through lpipm_upload_lockstep_shared_ub_eq: the blocks resident once, the slack
    block never formed on the host or the device.  Returns what solve_shared_matrix returns; x_slack has n + m_ub entries."""
    return _groups(lambda cx, b, c, c0: cx.upload_lockstep_shared_ub_eq(A_ub, A_eq, b, c, c0), bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def solve_shared_ub_tall(A_ub, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, duals=False, certificates=False):
    """Tall inequality-form LPs over ONE matrix (many right-hand sides or costs on one design matrix, A_ub x <= bs[i] with many
    more rows than columns): member i = (bs[i], cs[i] = the n structural costs, c0s[i]).  Lockstep groups of at most
    `max_group` on one context through lpipm_upload_lockstep_shared_ub_tall: A_ub and its transpose resident once, every member
    factoring its own n x n reduced system.  Returns what solve_shared_ub_eq returns; x_slack has n + m_ub entries."""
    return _groups(lambda cx, b, c, c0: cx.upload_lockstep_shared_ub_tall(A_ub, b, c, c0), bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def solve_shared_ub_eq_tall(A_ub, A_eq, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, duals=False, certificates=False):
    """Tall LPs with equality rows over ONE pair of blocks (solve_shared_ub_tall's users with a sum-to-one, budget or
    interpolation row): member i = (bs[i] = [b_ub_i; b_eq_i], cs[i] = the n structural costs, c0s[i]).  Lockstep groups of at
    most `max_group` on one context through lpipm_upload_lockstep_shared_ub_eq_tall: the image and the transpose of A_ub resident
    once, every member factoring its own n x n reduced system and its own m_eq x m_eq Schur complement.  Returns what
    solve_shared_ub_eq returns; x_slack has n + m_ub entries."""
    return _groups(lambda cx, b, c, c0: cx.upload_lockstep_shared_ub_eq_tall(A_ub, A_eq, b, c, c0), bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def sweep_chunks(count: int, max_group: int):
    """The equal chunks of a sweep: k = ceil(count / max_group) chunks of g = ceil(count / k) members, as lists of member
    indices.  The last chunk is filled up to g with repeats of its own last member (at most k - 1 of them in all), so
    every chunk after the first replaces the vectors of a resident batch of g instead of uploading a shorter one.
    -> (g, [indices of chunk 0, ...]); the first `count` indices in order are 0 .. count - 1."""
    if count < 1 or max_group < 1:
        return 0, []
    k = -(-count // max_group)
    g = -(-count // k)
    chunks = [list(range(q * g, min((q + 1) * g, count))) for q in range(k)]
    chunks[-1] += [chunks[-1][-1]] * (g - len(chunks[-1]))
    return g, chunks


def solve_device(A, b, c, c0s=None, *, form="slack", A_eq=None, n_slack=0, opts=None, ctx=None, max_group=32, duals=False, certificates=False):
    """A batch that is already on the GPU, end to end without a host copy of A, b, c or x: torch CUDA tensors as
    Context.upload_device takes them -- A [m, n] with b [K, .] (one matrix for all members) or A [K, m, n] (members that own
    their matrices), float64 or float32, any strides.  The members go through lockstep chunks of sweep_chunks's size (at most
    `max_group`), each uploaded from a slice of the tensors (lpipm_upload_device) and solved straight into its rows of the
    result (solve_lockstep_device).  A shared A is uploaded once per chunk size: a later chunk of the resident size only
    replaces the vectors (update_lockstep_vectors_device).
    -> (x, status, fun, iterations): x a float64 CUDA tensor [K, len(x)], NaN in the rows of members without a solution;
    status (int32), fun (float64, NaN without a solution) and iterations (int64) numpy arrays of K entries.
    duals=True: -> (x, status, fun, iterations, y, z, dual_fun) with y [K, len(b[i])] and z [K, len(x)] float64 CUDA tensors
    written by Context.duals_device after each chunk's solve (NaN rows for members without a solution) and dual_fun a numpy
    array (NaN likewise).
    certificates=True: the tuple gains (cert_y, cert_col, cert_kind) at its end -- cert_y [K, len(b[i])] and cert_col
    [K, len(x)] float64 CUDA tensors written by Context.certificates_device after each chunk's solve (the Farkas y and z of an
    infeasible member, the ray x of an unbounded one in cert_col; NaN rows for every other member) and cert_kind a numpy int32
    array (Context.certificate's kind)."""
    import torch
    import lp_amd
    _, _, K, nb, n_out, dev, batch = lp_amd._device_request(A, b, c, c0s, form, A_eq, n_slack)
    if not batch:
        raise lp_amd.IncompatibleInputDimensions()
    if max_group < 1:
        raise lp_amd.InvalidParameter("max_group must be >= 1")
    ctx = ctx or lp_amd.default_context(dev)
    opts = opts or lp_amd.InteriorPoint.default().opts()
    shared = A.ndim == 2
    x = torch.full((K, n_out), float("nan"), dtype=torch.float64, device=A.device)
    status, fun, its = np.zeros(K, dtype=np.int32), np.full(K, np.nan), np.zeros(K, dtype=np.int64)
    if duals:
        y = torch.full((K, nb), float("nan"), dtype=torch.float64, device=A.device)
        z = torch.full((K, n_out), float("nan"), dtype=torch.float64, device=A.device)
        dual_fun = np.full(K, np.nan)
        torch.cuda.current_stream(dev).synchronize()      # the fills run on torch's stream, the library on its own
    if certificates:
        cert_y = torch.full((K, nb), float("nan"), dtype=torch.float64, device=A.device)
        cert_col = torch.full((K, n_out), float("nan"), dtype=torch.float64, device=A.device)
        cert_kind = np.zeros(K, dtype=np.int32)
        torch.cuda.current_stream(dev).synchronize()
    g = sweep_chunks(K, max_group)[0]
    resident = 0                                          # members of the shared-matrix batch that is resident
    for k0 in range(0, K, g):
        k1 = min(k0 + g, K)
        c0 = None if c0s is None else [float(v) for v in c0s[k0:k1]]
        if shared and resident == k1 - k0:
            rows = lambda t: t[k0:k1] if t.dtype == torch.float64 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t[k0:k1].double().contiguous()
            bq, cq = rows(b), rows(c)
            torch.cuda.current_stream(dev).synchronize()
            ctx.update_lockstep_vectors_device(bq.data_ptr(), bq.stride(0), cq.data_ptr(), cq.stride(0), c0)
        else:
            ctx.upload_device(A if shared else A[k0:k1], b[k0:k1], c[k0:k1], c0, form=form, A_eq=A_eq, n_slack=n_slack)
            resident = k1 - k0 if shared else 0
        for i, (st, f, it) in enumerate(ctx.solve_lockstep_device(opts, x[k0].data_ptr(), n_out)):
            status[k0 + i], its[k0 + i] = st, it
            fun[k0 + i] = np.nan if f is None else f
        if duals:
            for i, (_, df) in enumerate(ctx.duals_device(y[k0].data_ptr(), nb, z[k0].data_ptr(), n_out)):
                dual_fun[k0 + i] = np.nan if df is None else df
        if certificates:
            for i, d in enumerate(ctx.certificates_device(cert_y[k0].data_ptr(), nb, cert_col[k0].data_ptr(), n_out)):
                cert_kind[k0 + i] = d["kind"]
    out = (x, status, fun, its) + ((y, z, dual_fun) if duals else ())
    return out + ((cert_y, cert_col, cert_kind) if certificates else ())


def _drive(chunks, upload, resident, bs, cs, c0s, opts, ctx, max_group, duals=False, certificates=False):
    """Member groups through lockstep batches on one context: `chunks(count, max_group)` gives the member indices of each group;
    group 0 is uploaded, a later one replaces the vectors of the resident batch (resident) or is uploaded in its turn."""
    import lp_amd
    count = len(bs)
    if len(cs) != count or (c0s is not None and len(c0s) != count):
        raise lp_amd.IncompatibleInputDimensions()
    if max_group < 1:
        raise lp_amd.InvalidParameter("max_group must be >= 1")
    ctx = ctx or lp_amd.default_context(0)
    opts = opts or lp_amd.InteriorPoint.default().opts()
    out = []
    for q, idx in enumerate(chunks(count, max_group)):
        pick = lambda seq: None if seq is None else [seq[i] for i in idx]
        if q == 0 or not resident:
            upload(ctx, pick(bs), pick(cs), pick(c0s))
        else:
            ctx.update_lockstep_vectors(pick(bs), pick(cs), pick(c0s))
        res = ctx.solve_lockstep(opts)
        first = len(out)
        for st, x, fun, it in res[:count - len(out)]:          # (a sweep's padding: its results are dropped)
            out.append(dict(status=st, x_slack=x, fun=fun, iterations=it))
        if duals:                                              # of this group's solve, before the next one replaces its iterate
            for member, d in zip(out[first:], ctx.duals_lockstep(len(out) - first)):   # (not a sweep's padding)
                member.update(y=d["y"] if d else None, z=d["z"] if d else None, dual_fun=d["dual_fun"] if d else None)
        if certificates and any(not lp_amd.has_x(q["status"]) for q in out[first:]):
            for member, d in zip(out[first:], ctx.certificates_lockstep(len(out) - first)):
                if not lp_amd.has_x(member["status"]):
                    member.update(cert_kind=d["kind"], cert_y=d["y"], cert_col=d["col"], cert_scale=d["scale"],
                                  cert_residual=d["residual"])
    return out


def _groups(upload, bs, cs, c0s, opts, ctx, max_group, duals=False, certificates=False):
    """Groups of at most max_group members in order, each uploaded."""
    return _drive(lambda count, g: [range(k, min(k + g, count)) for k in range(0, count, g)], upload, False,
                  bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def _sweep(upload, bs, cs, c0s, opts, ctx, max_group, duals=False, certificates=False):
    """The equal chunks of sweep_chunks: one upload, then new vectors for the resident batch."""
    return _drive(lambda count, g: sweep_chunks(count, g)[1], upload, True, bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def sweep_shared_matrix(A, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, n_slack=0, duals=False, certificates=False):
    """solve_shared_matrix for a sweep of more than one group: ONE upload_lockstep_shared (the first chunk), then
    update_lockstep_vectors for every later chunk -- A goes to the device once, and its first iteration's factor is formed
    once for the whole sweep.  The chunks are equal (sweep_chunks).  Returns what solve_shared_matrix returns, bit for bit."""
    return _sweep(lambda cx, b, c, c0: cx.upload_lockstep_shared(A, b, c, c0, n_slack=n_slack), bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def sweep_shared_ub_eq(A_ub, A_eq, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, duals=False, certificates=False):
    """solve_shared_ub_eq as a sweep: one upload_lockstep_shared_ub_eq, then update_lockstep_vectors per later chunk (bs[i] =
    [b_ub_i; b_eq_i], cs[i] = the n structural costs).  Returns what solve_shared_ub_eq returns, bit for bit."""
    return _sweep(lambda cx, b, c, c0: cx.upload_lockstep_shared_ub_eq(A_ub, A_eq, b, c, c0), bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def sweep_shared_ub_tall(A_ub, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, duals=False, certificates=False):
    """solve_shared_ub_tall as a sweep: one upload_lockstep_shared_ub_tall, then update_lockstep_vectors per later chunk (bs[i]
    of m_ub entries, cs[i] = the n structural costs); A_ub is uploaded and transposed once.  Returns what solve_shared_ub_tall
    returns, bit for bit."""
    return _sweep(lambda cx, b, c, c0: cx.upload_lockstep_shared_ub_tall(A_ub, b, c, c0), bs, cs, c0s, opts, ctx, max_group, duals, certificates)


def sweep_shared_ub_eq_tall(A_ub, A_eq, bs, cs, c0s=None, opts=None, ctx=None, max_group=32, duals=False, certificates=False):
    """solve_shared_ub_eq_tall as a sweep: one upload_lockstep_shared_ub_eq_tall, then update_lockstep_vectors per later chunk
    (bs[i] = [b_ub_i; b_eq_i], cs[i] = the n structural costs); the image is uploaded and A_ub transposed once.  Returns what
    solve_shared_ub_eq_tall returns, bit for bit."""
    return _sweep(lambda cx, b, c, c0: cx.upload_lockstep_shared_ub_eq_tall(A_ub, A_eq, b, c, c0), bs, cs, c0s, opts, ctx, max_group, duals, certificates)
