"""One form of the iteration tail per process, for a kernel trace of its launches (profiles/iteration_tail.md section 2):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/tail_forms.py FORM
then scripts/trace_launches.py over DIR (one file per process: the column split has three).  Run from the root of the tree under test; the problems are those of
tests/golden/make_iteration_tail.py.  `tail_forms.py --list` prints the forms."""
import os
import sys

sys.path.append(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
import make_iteration_tail as T  # noqa: E402
sys.path.insert(0, os.getcwd())                   # lp_amd of the tree under test, whichever tree this script lies in


def dense(m, n, seed=0, solves=1, **kw):
    def run(lp_amd):
        from lp_amd import synth
        ctx = lp_amd.Context(0)
        ctx.upload_arrays(*synth.planted_lp(seed, m, n)[:3])
        return [ctx.solve_raw(T.opts(**kw))[0] for _ in range(solves)]
    return run


def tall(me):
    def run(lp_amd):
        ctx = lp_amd.Context(0)
        p = T.tall_problem(3 if me else 2, 600, 40, me)
        ctx.upload_tall_eq(p) if me else ctx.upload(p, tall=True)
        return [ctx.solve_raw(T.opts())[0]]
    return run


def shared_tall_eq(lp_amd):
    X, _, Ae, _, _ = T.planted_eq(3, 600, 40, 5)
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared_ub_eq_tall(X, Ae, *T.shared_vectors(4, X, Ae, 3))
    return [m[0] for m in ctx.solve_lockstep(T.opts())]


def owned_tall(lp_amd):
    own = [T.planted_eq(10 + i, 600, 40, 0) for i in range(3)]
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_ub_tall([o[0] for o in own], [o[1] for o in own], [o[4] for o in own])
    return [m[0] for m in ctx.solve_lockstep(T.opts())]


def shared_dense(lp_amd):
    from lp_amd import synth
    A = synth.planted_lp(0, 200, 300)[0]
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep_shared(A, *T.dense_shared_vectors(5, A, 3))
    return [m[0] for m in ctx.solve_lockstep(T.opts())]


def lockstep16(lp_amd):
    from lp_amd import synth
    lock = [synth.planted_lp(20 + i, 130, 260)[:3] for i in range(16)]
    ctx = lp_amd.Context(0)
    ctx.upload_lockstep([l[0] for l in lock], [l[1] for l in lock], [l[2] for l in lock])
    return [m[0] for m in ctx.solve_lockstep(T.opts())]


# form -> (environment knobs, run)
FORMS = {
    "dense_two_solves": ({}, dense(200, 300, solves=2)),
    "dense_refine2": ({"LPIPM_REFINE": "2"}, dense(200, 300)),
    "dense_inverse": ({}, dense(200, 300, solver_type=1)),
    "dense_least_squares": ({}, dense(200, 300, solver_type=2)),
    "dense_unfused": ({"LPIPM_VEC_FUSED": "0"}, dense(200, 300)),
    "dense_130x1300": ({}, dense(130, 1300, seed=1)),
    "dense_1536x3072_lookahead1": ({"LPIPM_LOOKAHEAD": "1"}, dense(1536, 3072)),
    "tall": ({}, tall(0)),
    "tall_eq": ({}, tall(5)),
    "shared_tall_eq_3": ({}, shared_tall_eq),
    "owned_tall_3": ({}, owned_tall),
    "shared_dense_3": ({}, shared_dense),
    "lockstep_16": ({}, lockstep16),
    "colsplit_2": ({}, lambda lp_amd: [r[0] for r in T.column_split(0, 256, 512)]),
}

if __name__ == "__main__":
    if sys.argv[1:] == ["--list"]:
        print(" ".join(FORMS))
        sys.exit(0)
    knobs, run = FORMS[sys.argv[1]]
    if knobs:
        os.environ.update(knobs, LPIPM_EXPERIMENTAL="1")
    import lp_amd
    print(sys.argv[1], "statuses", run(lp_amd))
