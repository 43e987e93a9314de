"""What a failed or over-run solve may leave behind on a context, without a device: the inputs of
tests/test_gpu_after_a_failed_solve.py live here, and the ways that file dirties a context are shown to do what they claim on
the CPU oracle -- an input on which the oracle itself does not end as the GPU file needs fails in this file.

The ways: an over-run (tol = 1e-30, max_iter = 200: no exit test can pass, the iterate runs into the boundary until a pivot or
the NaN check ends the solve), an infeasible problem reached through new vectors alone, the iteration limit, and one loop body
from an iterate that holds a NaN or a zero.

Families (a family is the matrices of its members and named sets of vectors over them: "good", where the forms take new vectors
"alt" -- another good LP per member -- and "bad" -- an infeasible one):
  dense    synth.planted_lp / planted_scenarios; `augmented`: A2 = [A; 1^T], b2 = [b; sum x*], infeasible with b2' = [b; -1]
  slack    the scenario family of tests/test_gpu_slack_batches.py on blocks whose row 0 of A_ub is >= 0 (b[0] = -1: infeasible)
  tall     planted of tests/test_gpu_tall_form.py; the members of tests/test_gpu_tall_batches.py / test_gpu_tall_own_batches.py
  tall_eq  planted_eq of tests/test_tall_eq_host.py; the members of tests/test_tall_eq_batch_host.py"""
import functools
from typing import NamedTuple

import numpy as np
import pytest

import test_gpu_slack_batches as slack_gen              # (the generators of these files: nothing of them runs on a device here)
import test_gpu_tall_batches as tall_shared_gen
import test_gpu_tall_form as tall_gen
import test_gpu_tall_own_batches as tall_own_gen
from test_tall_eq_batch_host import BASE, member_of, pair_of
from test_tall_eq_host import _solve_np, make_tall_eq_solver, planted_eq

OK, NUMERICAL_PROBLEM, INFEASIBLE, ITERATION_LIMIT = 0, 2, 5, 7
OVERRUN = (("tol", 1e-30), ("max_iter", 200))
LIMIT = (("max_iter", 3),)


class Family(NamedTuple):
    kind: str           # "dense" | "slack" | "tall" | "tall_eq"
    shared: bool        # one set of matrices for all members
    mats: tuple         # per member (once when shared): dense (A,); slack and tall_eq (A_ub, A_eq); tall (X,)
    vecs: dict          # name -> (bs, cs), one entry per member; b = [b_ub; b_eq], c the structural costs (dense: of all columns)

    @property
    def count(self):
        return len(self.vecs["good"][0])

    def mat(self, i):
        return self.mats[0 if self.shared else i]

    def explicit(self, which, i):
        """Member i with the vectors `which` as the slack-form (A, b, c) the oracle solves."""
        b, c = self.vecs[which][0][i], self.vecs[which][1][i]
        if self.kind == "dense":
            return self.mat(i)[0], b, c
        A_ub, A_eq = self.mat(i) if self.kind != "tall" else (self.mat(i)[0], np.zeros((0, self.mat(i)[0].shape[1])))
        return slack_gen._explicit(A_ub, A_eq), b, slack_gen._pad(c, A_ub.shape[0])


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _first_row_negative(bs):
    """b[0] = -1 on every member: with row 0 of the `ub` block >= 0 and x >= 0 no point satisfies row 0."""
    out = [b.copy() for b in bs]
    for b in out:
        b[0] = -1.0
    return out


@functools.lru_cache(maxsize=None)
def dense(seed, m, n, count=1, shared=False, augmented=False):
    """count members of planted LPs: with matrices of their own (planted_lp(seed + i); "alt" a scenario on the same matrix), or
    scenarios on ONE matrix.  augmented: the extra row 1^T x = sum x*, which x* meets; "bad" asks for 1^T x = -1."""
    from lp_amd import synth
    if shared:
        A, bs, cs, xs = synth.planted_scenarios(seed, m, n, 2 * count)
        mats, good, alt = [A], (bs[:count], cs[:count], xs[:count]), (bs[count:], cs[count:], xs[count:])
    else:
        own = [synth.planted_lp(seed + i, m, n) for i in range(count)]
        other = [synth.planted_scenarios(seed + i, m, n, 1) for i in range(count)]
        mats = [p[0] for p in own]
        good = ([p[1] for p in own], [p[2] for p in own], [p[3] for p in own])
        alt = ([s[1][0] for s in other], [s[2][0] for s in other], [s[3][0] for s in other])
    vecs = {"good": good[:2], "alt": alt[:2]}
    if augmented:
        mats = [np.vstack([A, np.ones(n)]) for A in mats]
        ext = lambda bs, last: [np.concatenate([b, [v]]) for b, v in zip(bs, last)]
        vecs = {"good": (ext(good[0], [x.sum() for x in good[2]]), good[1]), "alt": (ext(alt[0], [x.sum() for x in alt[2]]), alt[1]),
                "bad": (ext(good[0], [-1.0] * count), good[1])}
    for bs, cs in vecs.values():
        _frozen(*bs, *cs)
    return Family("dense", shared, tuple((_frozen(A)[0],) for A in mats), vecs)


@functools.lru_cache(maxsize=None)
def slack(nx, m_ub, m_eq, count=1, shared=False):
    """count members of the scenario family of tests/test_gpu_slack_batches.py (its _blocks and _member), on blocks of their own or
    on ONE pair of blocks; row 0 of every A_ub is made >= 0."""
    mats, good, alt = [], ([], []), ([], [])
    for i in range(count):
        if not mats or not shared:
            A_ub, A_eq = slack_gen._blocks(np.random.default_rng([7, nx, m_ub, m_eq, i]), nx, m_ub, m_eq)
            A_ub[0, :] = np.abs(A_ub[0, :])
            mats.append(_frozen(A_ub, A_eq))
        rng = np.random.default_rng([8, nx, m_ub, m_eq, i])
        for dst in (good, alt):
            b, c = slack_gen._member(rng, *mats[-1])
            dst[0].append(b); dst[1].append(c)
    vecs = {"good": good, "alt": alt, "bad": (_first_row_negative(good[0]), good[1])}
    for bs, cs in vecs.values():
        _frozen(*bs, *cs)
    return Family("slack", shared, tuple(mats), vecs)


@functools.lru_cache(maxsize=None)
def tall(m, nx, count=0, shared=False):
    """count 0: the single LP planted(1, m, nx) of tests/test_gpu_tall_form.py, which takes no new vectors; else the members
    0 .. count - 1 ("alt": count .. 2 count - 1) of the shared-matrix or the own-matrix batch files at (m, nx)."""
    shape = (m, nx)
    if count == 0:
        X, b, c, _ = tall_gen.planted(1, m, nx)
        return Family("tall", False, (_frozen(X),), {"good": ([_frozen(b)[0]], [_frozen(c)[0]])})
    if shared:
        mats = (( tall_shared_gen._X(shape),),)
        pick = lambda first: tuple(list(v) for v in zip(*[tall_shared_gen._member(shape, first + i) for i in range(count)]))
    else:
        mats = tuple((tall_own_gen._X(shape, i),) for i in range(count))
        pick = lambda first: tuple(list(v) for v in zip(*[tall_own_gen._member(shape, (i, tall_own_gen.PLAIN, first + i)) for i in range(count)]))
    good, alt = pick(0), pick(count)
    bad = (list(_frozen(*_first_row_negative(good[0]))), good[1])
    return Family("tall", shared, mats, {"good": good, "alt": alt, "bad": bad})


@functools.lru_cache(maxsize=None)
def tall_eq(m, nx, me, count=0):
    """count 0: the single LP planted_eq(1, m, nx, me), which takes no new vectors; else members of the batch file's shape."""
    if count == 0:
        X, b, Ae, be, c, _ = planted_eq(1, m, nx, me)
        return Family("tall_eq", False, (_frozen(X, Ae),), {"good": ([_frozen(np.concatenate([b, be]))[0]], [_frozen(c)[0]])})
    shape = (m, nx, me)
    pick = lambda first: tuple(list(v) for v in zip(*[member_of(shape, first + i) for i in range(count)]))
    good, alt = pick(0), pick(count)
    bad = (list(_frozen(*_first_row_negative(good[0]))), good[1])
    return Family("tall_eq", True, (pair_of(shape),), {"good": good, "alt": alt, "bad": bad})


# ---- the families the GPU file uses -------------------------------------------------------------------------------------------------
# name -> (constructor, arguments).  Shapes: the smallest of each form's own test file with padding in every padded dimension and,
# where the form works in 128-blocks, more than one of them.
FAMILIES = {
    "dense-100x333": (dense, (1, 100, 333)),                         # mp 128
    "dense-130x300": (dense, (2, 130, 300)),                         # mp 256: two blocks
    "dense-130x300-x3": (dense, (2, 130, 300, 3)),                   # members with their own matrices
    "dense-100x333-shared3": (dense, (1, 100, 333, 3, True)),
    "dense-100x333-shared19": (dense, (1, 100, 333, 19, True)),      # two half-batch views of 9 and 10
    "slack-333+200+57": (slack, (333, 200, 57)),                     # m 257, mp 384
    "slack-333+200+57-x3": (slack, (333, 200, 57, 3)),
    "slack-333+200+57-shared3": (slack, (333, 200, 57, 3, True)),
    "tall-129x17": (tall, (129, 17)),
    "tall-520x130": (tall, (520, 130)),                              # nxp 256
    "tall-300x40-shared3": (tall, (300, 40, 3, True)),
    "tall-300x40-x3": (tall, (300, 40, 3)),
    "tall_eq-300x40+5": (tall_eq, BASE),                             # mep 16 > m_eq: the padding of Ve
    "tall_eq-300x40+39": (tall_eq, (300, 40, 39)),
    "tall_eq-300x40+5-shared3": (tall_eq, BASE + (3,)),
}
# ... and those of the `infeasible` route on the dense forms: the same LPs with the extra row
AUGMENTED = {
    "dense-101x333": (dense, (1, 100, 333, 1, False, True)),
    "dense-131x300-x3": (dense, (2, 130, 300, 3, False, True)),
    "dense-101x333-shared3": (dense, (1, 100, 333, 3, True, True)),
}
assert BASE == (300, 40, 5)


def family(name):
    make, args = {**FAMILIES, **AUGMENTED}[name]
    return make(*args)


def has_bad(name):
    """Whether the family has an infeasible set of vectors -- from its arguments alone, so that collecting a test builds nothing."""
    make, args = {**FAMILIES, **AUGMENTED}[name]
    return {dense: len(args) > 5 and args[5], slack: True, tall: len(args) > 2 and args[2] > 0, tall_eq: len(args) > 3}[make]


@functools.lru_cache(maxsize=None)
def oracle_status(name, which, i, kw=()):
    """(status, iterations) of the C oracle on member i of the family with the vectors `which`: computed once, shared."""
    from oracle import capi as oracle
    ref = oracle.solve(*family(name).explicit(which, i), opts=oracle.default_opts(**dict(kw)), want_log=False)
    return ref["status"], ref["iterations"]


def _members(names, which):
    return [(name, i) for name in names for i in range(family(name).count) if which in family(name).vecs]


# ---- the ways of dirtying a context do what they claim ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_overrun_is_a_numerical_problem(built, name):
    """tol = 1e-30 lets no exit test pass; within 200 iterations every LP the GPU file over-runs loses a pivot or fails the NaN
    check in the oracle.  On the tall forms the algebra the device runs -- K on the `ub` rows, the Schur complement on its factor
    -- emulated in numpy inside the oracle's loop ends the same way."""
    fam = family(name)
    for i in range(fam.count):
        st, it = oracle_status(name, "good", i, OVERRUN)
        print(f"\n[measure] over-run of {name} member {i}: oracle status {st} at iteration {it}")
        assert st == NUMERICAL_PROBLEM, (name, i, st, it)
        if fam.kind in ("tall", "tall_eq"):
            X = fam.mat(i)[0]
            got = _solve_np(*fam.explicit("good", i), OVERRUN, solver=make_tall_eq_solver(X.shape[1], X.shape[0]))
            print(f"[measure] over-run of {name} member {i}: emulated algebra status {got.status} at iteration {got.iterations}")
            assert got.status == NUMERICAL_PROBLEM, (name, i, got.status, got.iterations)


@pytest.mark.parametrize("name", list(FAMILIES) + list(AUGMENTED))
def test_the_vector_sets_end_as_their_names_say(built, name):
    """Every "good" and "alt" LP is Ok for the oracle, every "bad" one Infeasible, and "good" under max_iter = 3 is the
    iteration limit: the exits the GPU file's preconditions and follow-ups stand on."""
    fam = family(name)
    for which, want in (("good", OK), ("alt", OK), ("bad", INFEASIBLE)):
        for i in range(fam.count if which in fam.vecs else 0):
            st, it = oracle_status(name, which, i)
            print(f"\n[measure] {name} member {i} {which}: oracle status {st} in {it} iterations")
            assert st == want, (name, which, i, st, it)
    for i in range(fam.count):
        assert oracle_status(name, "good", i, LIMIT) == (ITERATION_LIMIT, 3), (name, i)


def poisoned_iterates(n, m):
    """The two starting points of the `nan_iterate` route: the blind start with x[0] = NaN, and with x[1] = 0 (D = x / z holds a
    zero, r_hat / x an inf).  -> [(name, x, y, z)]"""
    out = []
    for label, j, v in (("nan", 0, np.nan), ("zero", 1, 0.0)):
        x = np.ones(n); x[j] = v
        out.append((label, x, np.zeros(m), np.ones(n)))
    return out


@pytest.mark.parametrize("name", ["dense-100x333", "slack-333+200+57", "tall-129x17", "tall_eq-300x40+5"])
def test_one_iteration_from_a_poisoned_iterate_fails(built, name):
    """Ordinary NaN arithmetic, on the CPU as on the device: one loop body from such an iterate either fails in get_delta (the
    oracle stops at the pivot or at the NaN check, where the device goes on computing on NaNs) or returns a step that holds
    non-finite values."""
    from oracle import capi as oracle
    A, b, c = family(name).explicit("good", 0)
    for label, x, y, z in poisoned_iterates(A.shape[1], A.shape[0]):
        out = oracle.iteration(A, b, c, x, y, z, 1.0, 1.0)
        print(f"\n[measure] {name} from the {label} iterate: oracle status {out['status']}")
        assert out["status"] == NUMERICAL_PROBLEM or not np.isfinite(out["d_x"]).all(), (name, label, out["status"])
