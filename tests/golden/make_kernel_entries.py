"""Records what the kernel-granularity entries (the lpipm_k_* functions behind Context.k_*) return.

kernel_entries_parent.json : per case the exception class a call raised, or the SHA-256 of the bytes of every array and the
                             value of every integer it returned; never a time.  Plus the CU count of the device it was recorded
                             on (kernel plans, and with them the bits, depend on it).  tests/test_gpu_kernel_entries.py replays
                             every case on the code under test and requires equality.

The shapes are the smallest at which each branch of the entries is taken: m = 1, m = 128 (no padding), m = 200 (padding inside
one super-block) and m = 600 (mp = 640: two super-blocks of width 512) for the stand-alone factor entries, one and several
members for the lockstep ones, a dense, a slack-hinted, a `ub`+`eq` and a scaled resident problem, both tall forms, a tall
batch, a device upload of either form and a context with nothing resident.  lpipm_k_iteration is pinned by
iteration_tail_parent.json.  Of a matrix whose lower triangle alone is specified (k_adat, k_tall_normal, k_tall_schur) the lower
triangle is hashed.

The record is the behaviour of the commit it was taken at (the parent of the one that gave the entries one timer, one padded
copy and owned scratch buffers): regenerate it only at a commit whose results are the intended ones, never to make a failing
replay pass.  Only the public Python API is used, so the script runs unchanged at any commit that has it.  The record is taken
twice and written only if both runs agree.
Run from the repo root on an MI355X:  python tests/golden/make_kernel_entries.py
"""
import hashlib
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "kernel_entries_parent.json")

FACTOR_MS = (1, 128, 200, 600)
SPLITS = (0, 1, 99)


def _sha(a):
    a = np.ascontiguousarray(a)
    return a.dtype.str + ":" + hashlib.sha256(a.tobytes()).hexdigest()[:32]


def got(f):
    """What a call returned, or the class of what it raised."""
    try:
        return f()
    except Exception as e:          # noqa: BLE001  (the class is the record)
        return {"raises": type(e).__name__}


# ---------------------------------------------------------------- inputs
def spd(seed, m):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((m, m + 3))
    return G @ G.T / (m + 3) + np.eye(m)


def last_pivot_negative(seed, m):
    """Leading (m-1) x (m-1) block SPD, last pivot negative."""
    M = spd(seed, m)
    M[m - 1, m - 1] = -1.0
    return M


def rows(seed, nrhs, length):
    return np.random.default_rng(seed).standard_normal((nrhs, length))


def planted_blocks(seed, m, nx, me):
    """X (`ub` rows), b, A_eq, b_eq, c of a feasible, bounded inequality-form LP."""
    rng = np.random.default_rng(seed)
    X, Ae = rng.standard_normal((m, nx)), rng.standard_normal((me, nx))
    xs = rng.uniform(0.5, 1.5, nx)
    c = -X.T @ rng.uniform(0.5, 1.5, m) + Ae.T @ rng.standard_normal(me) + rng.uniform(0.5, 1.5, nx)
    return X, X @ xs + rng.uniform(0.5, 1.5, m), Ae, Ae @ xs, c


def problem(seed, m, nx, me):
    import lp_amd
    X, b, Ae, be, c = planted_blocks(seed, m, nx, me)
    p = lp_amd.Problem.target(c).ub(X, b)
    return (p.eq(Ae, be) if me else p).build()


def opts():
    import lp_amd
    return lp_amd.InteriorPoint.default().opts()


# ---------------------------------------------------------------- records of one entry
def potrf(ctx, M, repeats):
    L, info, _ = ctx.k_potrf(M, repeats=repeats)
    return [_sha(L), int(info)]


def inverses(ctx, m):
    inv, invT, w = ctx.k_factor_inverses(m)
    return [_sha(inv), _sha(invT), int(w)]


def qr(ctx, M, R):
    V, info, _ = ctx.k_qr_solve(M, R)
    return [_sha(V), int(info)]


def factor(ctx, m):
    """The stand-alone factor entries at size m, in the order that leaves a Cholesky factor for the solves."""
    M = spd(100 + m, m)
    rec = {"potrf:r1": got(lambda: potrf(ctx, M, 1)), "potrf:r3": got(lambda: potrf(ctx, M, 3)),
           "inverses": got(lambda: inverses(ctx, m))}
    for nrhs in (1, 2):
        R = rows(200 + m + nrhs, nrhs, m)
        for rep in (1, 3):
            rec[f"chol_solve:nrhs{nrhs}:r{rep}"] = got(lambda: _sha(ctx.k_chol_solve(m, R, repeats=rep)[0]))
        for s in SPLITS:
            rec[f"chol_solve_split:nrhs{nrhs}:split{s}"] = got(lambda: _sha(ctx.k_chol_solve_split(m, R, s)))
        V = rows(300 + m + nrhs, nrhs, m)
        rec[f"symv_residual:nrhs{nrhs}"] = got(lambda: _sha(ctx.k_symv_residual(M, V, R)))
    rec["chol_solve:after_symv_residual"] = got(lambda: _sha(ctx.k_chol_solve(m, rows(1, 1, m))[0]))
    for nrhs in (1, 2):
        rec[f"qr_solve:nrhs{nrhs}"] = got(lambda: qr(ctx, M, rows(400 + m + nrhs, nrhs, m)))
    rec["chol_solve:after_qr_solve"] = got(lambda: _sha(ctx.k_chol_solve(m, rows(1, 1, m))[0]))
    rec["chol_solve_split:after_qr_solve"] = got(lambda: _sha(ctx.k_chol_solve_split(m, rows(1, 1, m), 1)))
    rec["inverses:after_qr_solve"] = got(lambda: inverses(ctx, m))
    return rec


def not_spd(ctx):
    M = last_pivot_negative(7, 200)
    return {"potrf:r1": got(lambda: potrf(ctx, M, 1)), "potrf:r3": got(lambda: potrf(ctx, M, 3)),
            "chol_solve:never_factored_size": got(lambda: _sha(ctx.k_chol_solve(77, rows(1, 1, 77))[0]))}


def lockstep_matrices(m, count, bad):
    Ms = np.stack([spd(500 + m + q, m) for q in range(count)])
    if bad is not None:
        Ms[bad] = last_pivot_negative(600 + m, m)
    return Ms


def potrf_lockstep(ctx, m, count, bad=None):
    def run():
        L, infos = ctx.k_potrf_lockstep(lockstep_matrices(m, count, bad))
        return [_sha(L), [int(i) for i in infos]]
    return got(run)


def trsm_lockstep(ctx, count, nrows, cols, shared, masked, n=300):
    def run():
        B = rows(700 + nrows + cols, nrows if shared else count * nrows, cols)
        B = B if shared else B.reshape(count, nrows, cols)
        kw = dict(done_mask=[0, 1, 0], fill=7.0) if masked else {}
        Z, infos = ctx.k_trsm_lt_lockstep(lockstep_matrices(n, count, None), B, **kw)
        return [_sha(Z), [int(i) for i in infos]]
    return got(run)


def adat(ctx, dinv, repeats):
    return _sha(np.tril(ctx.k_adat(dinv, repeats=repeats)[0]))


def gemv_dual(ctx, w, v, repeats):
    Aw, ATv, _ = ctx.k_gemv_dual(w, v, repeats=repeats)
    return [_sha(Aw), _sha(ATv)]


def resident(ctx):
    """The entries that read the resident problem: A.D.A^T, the three GEMVs and the image itself."""
    rng = np.random.default_rng(40)
    dinv = rng.uniform(0.5, 2.0, ctx.n)
    rec = {"resident_matrix": got(lambda: _sha(ctx.k_resident_matrix(0)))}
    for rep in (1, 3):
        rec[f"adat:r{rep}"] = got(lambda: adat(ctx, dinv, rep))
        rec[f"gemv_dual:r{rep}"] = got(lambda: gemv_dual(ctx, rows(41, 1, ctx.n)[0], rows(42, 1, ctx.m)[0], rep))
        for nrhs in (1, 2):
            rec[f"gemv_n:nrhs{nrhs}:r{rep}"] = got(lambda: _sha(ctx.k_gemv_n(rows(43 + nrhs, nrhs, ctx.n), repeats=rep)[0]))
            rec[f"gemv_t:nrhs{nrhs}:r{rep}"] = got(lambda: _sha(ctx.k_gemv_t(rows(45 + nrhs, nrhs, ctx.m), repeats=rep)[0]))
    return rec


def tall_sym_solve(ctx, nrhs):
    dinv = np.random.default_rng(50).uniform(0.5, 2.0, ctx.n)
    U, V, info = ctx.k_tall_sym_solve(dinv, rows(51 + nrhs, nrhs, ctx.n), rows(53 + nrhs, nrhs, ctx.m))
    return [_sha(U), _sha(V), int(info)]


def tall(ctx, with_resident=True):
    """The tall entries on what is resident (refusals included), then, `with_resident`, the entries every upload has."""
    dinv = np.random.default_rng(50).uniform(0.5, 2.0, ctx.n)
    rec = {"tall_normal": got(lambda: _sha(np.tril(ctx.k_tall_normal(dinv)))),
           "tall_schur": got(lambda: _sha(np.tril(ctx.k_tall_schur(dinv))))}
    for nrhs in (1, 2):
        rec[f"tall_sym_solve:nrhs{nrhs}"] = got(lambda: tall_sym_solve(ctx, nrhs))
    if with_resident:
        rec.update(resident(ctx))
    return rec


def pack(ctx, upload, A, b, c, **kw):
    """[rc of the upload's launch run again, image before, image after]; a refusal is recorded with the image it left."""
    def run():
        upload(ctx)
        before = _sha(ctx.k_resident_matrix(0))
        packed = got(lambda: [bool(v > 0.0 and math.isfinite(v)) for v in ctx.k_pack_matrix(A, b, c, repeats=2, **kw)])
        return [packed, before, _sha(ctx.k_resident_matrix(0))]
    return got(run)


def no_problem(ctx):
    """Every entry on a context with nothing resident; the entries that need a factor first, before one exists."""
    one, two = np.ones(5), np.ones((2, 5))
    M = spd(9, 5)
    rec = {
        "chol_solve": got(lambda: _sha(ctx.k_chol_solve(5, one)[0])),
        "chol_solve_split": got(lambda: _sha(ctx.k_chol_solve_split(5, one, 1))),
        "factor_inverses": got(lambda: inverses(ctx, 5)),
        "resident_matrix": got(lambda: _sha(ctx.k_resident_matrix(0))),
        "adat": got(lambda: adat(ctx, one, 1)),
        "gemv_n": got(lambda: _sha(ctx.k_gemv_n(two)[0])),
        "gemv_t": got(lambda: _sha(ctx.k_gemv_t(two)[0])),
        "gemv_dual": got(lambda: gemv_dual(ctx, one, one, 1)),
        "iteration": got(lambda: int(ctx.k_iteration(opts(), one, one, one, 1.0, 1.0)["info"])),
        "tall_normal": got(lambda: _sha(ctx.k_tall_normal(one))),
        "tall_schur": got(lambda: _sha(ctx.k_tall_schur(one))),
        "tall_sym_solve": got(lambda: _sha(ctx.k_tall_sym_solve(one, two, two)[0])),
        "potrf": got(lambda: potrf(ctx, M, 1)),
        "symv_residual": got(lambda: _sha(ctx.k_symv_residual(M, two, two))),
        "qr_solve": got(lambda: qr(ctx, M, two)),
        "potrf_lockstep": potrf_lockstep(ctx, 5, 2),
        "trsm_lt_lockstep": trsm_lockstep(ctx, 2, 3, 5, True, False, n=5),
        "mfma_f64_probe": got(lambda: [bool(v > 0.0 and math.isfinite(v)) for v in ctx.k_mfma_f64_probe(iters=200)]),
    }
    import torch
    A = torch.ones((4, 6), dtype=torch.float64, device="cuda")
    b, c = torch.ones(4, dtype=torch.float64, device="cuda"), torch.ones(6, dtype=torch.float64, device="cuda")
    rec["pack_matrix"] = got(lambda: [bool(v > 0.0) for v in ctx.k_pack_matrix(A, b, c, repeats=1)])
    return rec


# ---------------------------------------------------------------- uploads
def dense_lp():
    from lp_amd import synth
    return synth.planted_lp(0, 70, 150)[:3]


def slack_lp():
    """70 x 150 whose last 70 columns are the slack block I."""
    X, b, _, _, c = planted_blocks(60, 70, 80, 0)
    return np.hstack([X, np.eye(70)]), b, np.concatenate([c, np.zeros(70)])


def up_dense(ctx):
    ctx.upload_arrays(*dense_lp())


def up_slack(ctx):
    ctx.upload_arrays(*slack_lp(), n_slack=70)


def up_ub_eq(ctx):
    ctx.upload(problem(61, 60, 90, 10))


def up_scaled(ctx):
    ctx.set_scaling(8)
    up_dense(ctx)


def up_tall(ctx):
    ctx.upload(problem(62, 300, 40, 0), tall=True)


def up_tall_eq(ctx):
    ctx.upload_tall_eq(problem(63, 300, 40, 5))


def up_tall_batch(ctx):
    own = [planted_blocks(64 + i, 300, 40, 0) for i in range(2)]
    ctx.upload_lockstep_ub_tall([o[0] for o in own], [o[1] for o in own], [o[4] for o in own])


def device_lps():
    """-> {label: (A, b, c, keywords of upload_device)} as float64 CUDA tensors: a slack-form LP and a tall one."""
    import torch
    T = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")
    A, b, c = slack_lp()
    X, bt, _, _, ct = planted_blocks(62, 300, 40, 0)
    return {"slack:70x150": (T(A), T(b), T(c), dict(n_slack=70)), "tall:300x40": (T(X), T(bt), T(ct), dict(form="ub_tall"))}


# ---------------------------------------------------------------- the cases
def on_context(body, upload=None):
    import lp_amd
    ctx = lp_amd.Context(0)
    try:
        if upload is not None:
            upload(ctx)
        return body(ctx)
    finally:
        ctx.close()


def cases():
    """-> {label: record}"""
    rec = {}

    def factors(ctx):                       # one context: the persistent scratch is regrown from size to size
        for m in FACTOR_MS:
            rec[f"factor:{m}"] = factor(ctx, m)
        rec["factor:200:last_pivot_negative"] = not_spd(ctx)
    on_context(factors)

    def locksteps(ctx):
        for m in (100, 300):
            for count in (1, 3):
                rec[f"potrf_lockstep:{m}x{count}"] = potrf_lockstep(ctx, m, count)
                rec[f"potrf_lockstep:{m}x{count}:member{count - 1}_not_spd"] = potrf_lockstep(ctx, m, count, bad=count - 1)
        for count in (1, 3):
            for nrows in (1, 17):
                for cols in (300, 297):
                    for shared in (True, False):
                        for masked in ((False, True) if count == 3 else (False,)):
                            label = f"trsm_lt_lockstep:300x{count}:{nrows}x{cols}:{'shared' if shared else 'own'}_b"
                            rec[label + (":masked" if masked else "")] = trsm_lockstep(ctx, count, nrows, cols, shared, masked)
    on_context(locksteps)

    rec["resident:dense:70x150"] = on_context(resident, up_dense)
    rec["resident:slack:70x150"] = on_context(resident, up_slack)
    rec["resident:ub_eq:60+10x90"] = on_context(resident, up_ub_eq)
    rec["resident:scaled:70x150"] = on_context(resident, up_scaled)
    rec["tall:300x40"] = on_context(tall, up_tall)
    rec["tall_eq:300x40+5"] = on_context(tall, up_tall_eq)
    rec["tall_entries:on_dense:70x150"] = on_context(lambda ctx: tall(ctx, False), up_dense)
    rec["tall_entries:on_tall_batch:2x300x40"] = on_context(lambda ctx: tall(ctx, False), up_tall_batch)

    for label, (A, b, c, kw) in device_lps().items():
        rec[f"pack_matrix:{label}"] = on_context(lambda ctx: pack(ctx, lambda cx: cx.upload_device(A, b, c, **kw), A, b, c, **kw))
        rec[f"pack_matrix:{label}:scaled"] = on_context(
            lambda ctx: pack(ctx, lambda cx: cx.set_scaling(8).upload_device(A, b, c, **kw), A, b, c, **kw))
    rec["mfma_f64_probe"] = on_context(lambda ctx: got(lambda: [bool(v > 0.0 and math.isfinite(v)) for v in ctx.k_mfma_f64_probe(iters=2000)]))
    rec["no_problem"] = on_context(no_problem)
    return json.loads(json.dumps(rec))


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def load(path=OUT):
    with open(path) as f:
        return json.load(f)


def leaves(rec, at=""):
    """{path: leaf} of a nested record, for a readable difference."""
    if isinstance(rec, dict):
        out = {}
        for k, v in rec.items():
            out.update(leaves(v, f"{at}/{k}"))
        return out
    return {at: rec}


def main():
    first, second = leaves(cases()), leaves(cases())
    differ = sorted(k for k in first if first[k] != second.get(k))
    assert not differ and sorted(first) == sorted(second), f"two runs on one commit differ in {differ}: nothing written"
    same = [k for k in first if k.endswith(":r3") and first[k] != first[k[:-1] + "1"]]
    assert not same, f"repeats = 3 and repeats = 1 return different arrays in {same}: nothing written"
    doc = dict(note="recorded by tests/golden/make_kernel_entries.py; per case and entry the class a call raised, or the sha256 of "
                    "the bytes of each array it returned (dtype first, cut to 32 hex digits) and its integers; no times",
               cu_count=cu_count(), cases=first)
    with open(OUT, "w") as f:
        f.write('{"note":%s,\n"cu_count":%d,\n"cases":{\n' % (json.dumps(doc["note"]), doc["cu_count"]))
        f.write(",\n".join("%s:%s" % (json.dumps(k), json.dumps(first[k], separators=(",", ":"))) for k in sorted(first)))
        f.write("\n}}\n")
    assert load() == json.loads(json.dumps(doc))
    print(len(first), "records, CU count", doc["cu_count"], "taken twice, identical")
    for k in sorted(first):
        print(k, json.dumps(first[k])[:150])


if __name__ == "__main__":
    main()
