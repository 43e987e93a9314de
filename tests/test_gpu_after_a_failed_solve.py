"""A failed or over-run solve leaves nothing behind.

The contract: after ANY earlier activity on a context, a solve of the resident problem is BIT-IDENTICAL to that solve on a fresh
context with the same upload and settings -- status, iteration count, the bits of x and of fun, and every row of the iteration
log where the entry point returns one -- with or without new vectors in between.  A solve does not clear the arena the upload
sized: it resets the iterate and relies on every other buffer being rewritten before it is read, and on the padding past m, n,
nx and m_eq still being zero.  This file dirties a context and then asks for the good solve.

Ways to dirty a context, each with its precondition asserted (tests/test_after_a_failed_solve_host.py shows them on the oracle):
  overrun     tol = 1e-30, max_iter = 200: every member ends in NumericalProblem, with NaNs behind its lost pivot
  nan, zero   one loop body (k_iteration; single uploads) from an iterate with x[0] = NaN, or x[1] = 0: a step that is not finite
  infeasible  new vectors that make every member infeasible (the forms that take new vectors)
  limit       max_iter = 3
Follow-ups, the context dirtied anew in front of each: (a) the same LP under the default options, (b) new vectors for another good
LP over the same matrix, (c) ip = 0, (d) on the single m x m forms the other arm: the QR solver types after a dirtied Cholesky
solve and the reverse.  The references are fresh contexts, computed once per (form, vectors, options, settings) and shared.

The families of LPs and their shapes: tests/test_after_a_failed_solve_host.py."""
import functools
from typing import Callable, NamedTuple, Optional

import numpy as np
import pytest

import test_after_a_failed_solve_host as host
from test_after_a_failed_solve_host import INFEASIBLE, ITERATION_LIMIT, LIMIT, NUMERICAL_PROBLEM, OK, OVERRUN, family, poisoned_iterates

pytestmark = pytest.mark.gpu

REFINING = (("LPIPM_EXPERIMENTAL", "1"), ("LPIPM_REFINE", "2"))
ONE_STREAM = (("LPIPM_EXPERIMENTAL", "1"), ("LPIPM_HALVES", "0"))
QR_TYPES = (1, 2)                 # EquationSolverType.Inverse, .LeastSquares


def _opts(**kw):
    import lp_amd
    o = lp_amd.InteriorPoint.default().opts()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


# ---- the forms ----------------------------------------------------------------------------------------------------------------------
def _explicit(fam, which):
    """Every member in the explicit slack form: -> As, bs, cs (all columns)."""
    ms = [fam.explicit(which, i) for i in range(fam.count)]
    return [m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms]


def _up_plain(cx, fam, which):
    cx.upload_arrays(*fam.explicit(which, 0))


def _up_hint(cx, fam, which):
    cx.upload_arrays(*fam.explicit(which, 0), 0.0, fam.mat(0)[0].shape[0])


def _new_single(cx, fam, which):
    _, b, c = fam.explicit(which, 0)
    cx.update_vectors(b, c)


def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(torch.device("cuda", 0))      # (a copy: the families are read-only)


def _up_device(cx, fam, which):
    cx.upload_device(*[_cuda(a) for a in fam.explicit(which, 0)])


def _new_single_device(cx, fam, which):
    _, b, c = fam.explicit(which, 0)
    cx.update_vectors_device(_cuda(b), _cuda(c))


def _problem(fam, which):
    import lp_amd
    b, c = fam.vecs[which][0][0], fam.vecs[which][1][0]
    mats = fam.mat(0)
    m_ub = mats[0].shape[0]
    p = lp_amd.Problem.target(c).ub(mats[0], b[:m_ub])
    return (p.eq(mats[1], b[m_ub:]) if len(mats) > 1 and mats[1].shape[0] else p).build()


def _up_parts(cx, fam, which):
    cx.upload(_problem(fam, which))


def _up_tall(cx, fam, which):
    cx.upload(_problem(fam, which), tall=True)


def _up_tall_eq(cx, fam, which):
    cx.upload_tall_eq(_problem(fam, which))


def _up_lockstep(cx, fam, which):
    cx.upload_lockstep(*_explicit(fam, which))


def _up_lockstep_hint(cx, fam, which):
    cx.upload_lockstep(*_explicit(fam, which), None, fam.mat(0)[0].shape[0])


def _up_shared(cx, fam, which):
    _, bs, cs = _explicit(fam, which)
    cx.upload_lockstep_shared(fam.explicit(which, 0)[0], bs, cs)


def _up_shared_hint(cx, fam, which):
    _, bs, cs = _explicit(fam, which)
    cx.upload_lockstep_shared(fam.explicit(which, 0)[0], bs, cs, None, fam.mat(0)[0].shape[0])


def _new_explicit(cx, fam, which):
    _, bs, cs = _explicit(fam, which)
    cx.update_lockstep_vectors(bs, cs)


def _up_shared_ub_eq(cx, fam, which):
    cx.upload_lockstep_shared_ub_eq(*fam.mat(0), *fam.vecs[which])


def _up_shared_ub_tall(cx, fam, which):
    cx.upload_lockstep_shared_ub_tall(fam.mat(0)[0], *fam.vecs[which])


def _up_own_ub_tall(cx, fam, which):
    cx.upload_lockstep_ub_tall([fam.mat(i)[0] for i in range(fam.count)], *fam.vecs[which])


def _up_shared_ub_eq_tall(cx, fam, which):
    cx.upload_lockstep_shared_ub_eq_tall(*fam.mat(0), *fam.vecs[which])


def _new_parts(cx, fam, which):
    cx.update_lockstep_vectors(*fam.vecs[which])


class Form(NamedTuple):
    family: str
    upload: Callable
    new_vectors: Optional[Callable] = None      # None: the form takes no new vectors
    batch: bool = False
    augmented: Optional[str] = None             # dense forms: the family of the `infeasible` route (its matrix has one more row)
    square: bool = False                        # a single m x m form: the QR arms, k_adat and k_gemv_dual apply
    knobs: tuple = ()                           # in the environment while the context is created


FORMS = {
    "plain-100x333": Form("dense-100x333", _up_plain, _new_single, augmented="dense-101x333", square=True),
    "plain-130x300": Form("dense-130x300", _up_plain, _new_single, square=True),
    "plain-refining": Form("dense-130x300", _up_plain, _new_single, square=True, knobs=REFINING),
    "slack-hint": Form("slack-333+200+57", _up_hint, _new_single, square=True),
    "ub_eq-parts": Form("slack-333+200+57", _up_parts, square=True),
    "tall-129x17": Form("tall-129x17", _up_tall),
    "tall-520x130": Form("tall-520x130", _up_tall),
    "tall_eq-300x40+5": Form("tall_eq-300x40+5", _up_tall_eq),
    "tall_eq-300x40+39": Form("tall_eq-300x40+39", _up_tall_eq),
    "device-plain": Form("dense-100x333", _up_device, _new_single_device, augmented="dense-101x333", square=True),
    "lockstep-3": Form("dense-130x300-x3", _up_lockstep, _new_explicit, batch=True, augmented="dense-131x300-x3"),
    "lockstep-slack-3": Form("slack-333+200+57-x3", _up_lockstep_hint, _new_explicit, batch=True),
    "shared-3": Form("dense-100x333-shared3", _up_shared, _new_explicit, batch=True, augmented="dense-101x333-shared3"),
    "shared-19": Form("dense-100x333-shared19", _up_shared, _new_explicit, batch=True),
    "shared-19-one-stream": Form("dense-100x333-shared19", _up_shared, _new_explicit, batch=True, knobs=ONE_STREAM),
    "shared-slack-3": Form("slack-333+200+57-shared3", _up_shared_hint, _new_explicit, batch=True),
    "shared-ub_eq-3": Form("slack-333+200+57-shared3", _up_shared_ub_eq, _new_parts, batch=True),
    "shared-ub_tall-3": Form("tall-300x40-shared3", _up_shared_ub_tall, _new_parts, batch=True),
    "own-ub_tall-3": Form("tall-300x40-x3", _up_own_ub_tall, _new_parts, batch=True),
    "shared-ub_eq_tall-3": Form("tall_eq-300x40+5-shared3", _up_shared_ub_eq_tall, _new_parts, batch=True),
}
SINGLES = [k for k, f in FORMS.items() if not f.batch]
DEFAULTS = (True, 0)              # settings: (first-factor cache, scaling passes) -- the library's defaults


def _context(form, settings=DEFAULTS):
    import lp_amd
    with pytest.MonkeyPatch.context() as mp:
        for k, v in form.knobs:
            mp.setenv(k, v)
        cx = lp_amd.Context(0)
    cache, passes = settings
    if not cache:
        cx.set_first_factor_cache(False)
    if passes:
        cx.set_scaling(passes)
    return cx


def _solve(cx, form, kw=()):
    """Single: (status, bits of x | None, bits of fun | None, iterations, bits of the log).  Batch: one such tuple per member,
    without a log."""
    has_x = lambda rc: rc in (OK, ITERATION_LIMIT)
    if form.batch:
        return [(int(rc), _bits(x) if has_x(rc) else None, _bits(fun) if has_x(rc) else None, int(it))
                for rc, x, fun, it in cx.solve_lockstep(_opts(**dict(kw)))]
    rc, x, fun, it, rows = cx.solve_raw(_opts(**dict(kw)), want_log=True)
    return [(int(rc), _bits(x) if has_x(rc) else None, _bits(fun) if has_x(rc) else None, int(it), _bits(np.array(rows)))]


def _statuses(res):
    return [r[0] for r in res]


@functools.lru_cache(maxsize=None)
def _fresh(name, fam_name, which, kw=(), settings=DEFAULTS):
    """The solve on a fresh context: computed once, shared, immutable."""
    form = FORMS[name]
    cx = _context(form, settings)
    form.upload(cx, family(fam_name), which)
    out = tuple(_solve(cx, form, kw))
    cx.close()
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g[0], g[3]) == (w[0], w[3]), (what, f"member {i}: status {g[0]} in {g[3]} iterations, fresh {w[0]} in {w[3]}")
        assert g[2] == w[2], (what, i, "fun")
        assert g[1] == w[1], (what, i, "x")
        assert g[4:] == w[4:], (what, i, "log")


# ---- the ways to dirty a context ------------------------------------------------------------------------------------------------------
def _dirty(cx, form, fam, route, kw=()):
    """One dirtying step with its precondition.  kw: further options (the solver type of follow-up (d))."""
    if route == "overrun":
        st = _statuses(_solve(cx, form, OVERRUN + kw))
        assert st == [NUMERICAL_PROBLEM] * fam.count, (route, st)
    elif route == "limit":
        st = _statuses(_solve(cx, form, LIMIT + kw))
        assert st == [ITERATION_LIMIT] * fam.count, (route, st)
    elif route == "infeasible":
        form.new_vectors(cx, fam, "bad")
        st = _statuses(_solve(cx, form, kw))
        assert st == [INFEASIBLE] * fam.count, (route, st)
    else:
        x, y, z = {label: it for label, *it in poisoned_iterates(cx.n, cx.m)}[route]
        out = cx.k_iteration(_opts(**dict(kw)), x, y, z, 1.0, 1.0)
        assert not np.isfinite(out["d_x"]).all(), route


def _routes(form):
    routes = ["overrun", "limit"] + ([] if form.batch else ["nan", "zero"])
    return routes + (["infeasible"] if host.has_bad(form.family) and form.new_vectors else [])


def _cases():
    """(form, family, route): every route on the form's family; on the dense forms `infeasible` on the family with the extra row."""
    out = []
    for name, form in FORMS.items():
        out += [(name, form.family, r) for r in _routes(form)]
        if form.augmented:
            out.append((name, form.augmented, "infeasible"))
    return out


CASES = _cases()


@pytest.mark.parametrize("name,fam_name,route", CASES, ids=[f"{n}-{r}" for n, _, r in CASES])
def test_the_good_solve_after_a_dirtied_context(built, name, fam_name, route):
    form, fam = FORMS[name], family(fam_name)
    cx = _context(form)
    form.upload(cx, fam, "good")

    def again(which="good"):
        """The vectors of the follow-up: other ones, or the good ones back where the route has replaced them."""
        if which != "good" or route == "infeasible":
            form.new_vectors(cx, fam, which)

    _dirty(cx, form, fam, route)                                                    # (a) the same LP, default options
    again()
    _assert_same(_solve(cx, form), _fresh(name, fam_name, "good"), f"{name} after {route}: (a) the same LP")
    if form.new_vectors is not None:                                                # (b) another good LP over the same matrix
        _dirty(cx, form, fam, route)
        again("alt")
        _assert_same(_solve(cx, form), _fresh(name, fam_name, "alt"), f"{name} after {route}: (b) new vectors")
        form.new_vectors(cx, fam, "good")
    _dirty(cx, form, fam, route)                                                    # (c) ip = 0
    again()
    _assert_same(_solve(cx, form, (("ip", 0),)), _fresh(name, fam_name, "good", (("ip", 0),)), f"{name} after {route}: (c) ip = 0")
    if form.square and not form.knobs:                                              # (d) the other arm
        for st in QR_TYPES:
            kw = (("solver_type", st),)
            _dirty(cx, form, fam, route)
            again()
            _assert_same(_solve(cx, form, kw), _fresh(name, fam_name, "good", kw), f"{name} after {route}: (d) Cholesky, then type {st}")
            if route != "overrun":             # (the over-run's precondition is the Cholesky arm's lost pivot)
                _dirty(cx, form, fam, route, kw)
                again()
                _assert_same(_solve(cx, form), _fresh(name, fam_name, "good"), f"{name} after {route}: (d) type {st}, then Cholesky")
    cx.close()


@pytest.mark.parametrize("name", list(FORMS))
def test_the_fresh_results_have_the_oracles_status(built, name):
    """The references above are the project's own: once per form they are held against the oracle's exits, so that two equally
    wrong solves do not pass."""
    form = FORMS[name]
    for fam_name in [form.family] + ([form.augmented] if form.augmented else []):
        fam = family(fam_name)
        for which in fam.vecs if form.new_vectors else ["good"]:
            want = [host.oracle_status(fam_name, which, i)[0] for i in range(fam.count)]
            assert _statuses(_fresh(name, fam_name, which)) == want, (name, fam_name, which)
        assert _statuses(_fresh(name, fam_name, "good", LIMIT)) == [host.oracle_status(fam_name, "good", i, LIMIT)[0] for i in range(fam.count)]


# ---- settings: the first-factor cache and the scaling -----------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", [0, 8], ids=["unscaled", "scaled8"])
@pytest.mark.parametrize("cache", [True, False], ids=["cache-on", "cache-off"])
@pytest.mark.parametrize("name", ["plain-130x300", "tall-520x130"])
def test_settings(built, name, cache, passes):
    """One m x m and one tall shape under every setting that changes what a context keeps: each route, then the same LP under the
    default options and under ip = 0, against a fresh context with the same settings.  With the cache on the kept first factor is
    still the one replayed -- one A.D.A^T launch fewer than iterations -- and still right: the bits are those of the cache-off
    reference as well."""
    form, fam = FORMS[name], family(FORMS[name].family)
    settings = (cache, passes)
    cx = _context(form, settings)
    cx.set_profiling(2)
    form.upload(cx, fam, "good")
    first = _solve(cx, form)
    _assert_same(first, _fresh(name, form.family, "good", (), settings), f"{name} {settings}: first solve")
    for route in _routes(form):
        for kw in ((), (("ip", 0),)):
            _dirty(cx, form, fam, route)
            got = _solve(cx, form, kw)
            _assert_same(got, _fresh(name, form.family, "good", kw, settings), f"{name} {settings} after {route}: {kw}")
            _assert_same(got, _fresh(name, form.family, "good", kw, (False, passes)), f"{name} {settings} after {route}: {kw}, cache-off reference")
            t = cx.phase_times()
            if form.square:              # (a tall upload keeps no factor)
                assert t["adat_launches"] == t["iterations"] - (1 if cache else 0), (name, settings, route, t["adat_launches"], t["iterations"])
    cx.close()


# ---- the kernel entries share the arena's vectors with the solve ------------------------------------------------------------------------
def _kernel_outputs(cx, form, fam, check=False):
    """The outputs of every kernel entry the form has, as bits.  check (the fresh reference): they are finite."""
    rng = np.random.default_rng(5)
    n, m = cx.n, cx.m
    dinv = rng.uniform(0.5, 2.0, n)
    out = {}
    if form.square:
        M, _ = cx.k_adat(dinv)
        out["k_adat"] = _bits(np.tril(M))
        Aw, ATv, _ = cx.k_gemv_dual(rng.standard_normal(n), rng.standard_normal(m))
        out["k_gemv_dual"] = _bits(Aw) + _bits(ATv)
        G = rng.standard_normal((m, 2 * m))
        L, info, _ = cx.k_potrf(G @ G.T / (2 * m) + np.eye(m))
        assert info == 0
        V = cx.k_chol_solve(m, rng.standard_normal((2, m)))[0]
        assert not check or (np.isfinite(M).all() and np.isfinite(Aw).all() and np.isfinite(ATv).all() and np.isfinite(V).all())
        out["k_chol_solve"] = _bits(np.tril(L)) + _bits(V)
    else:
        out["k_tall_normal"] = _bits(np.tril(cx.k_tall_normal(dinv)))
        for nrhs in (1, 2):
            U, V, info = cx.k_tall_sym_solve(dinv, rng.standard_normal((nrhs, n)), rng.standard_normal((nrhs, m)))
            assert not check or (info == 0 and np.isfinite(U).all() and np.isfinite(V).all())
            out[f"k_tall_sym_solve-{nrhs}"] = _bits(U) + _bits(V) + bytes([info == 0])
        if cx._m_eq:
            out["k_tall_schur"] = _bits(np.tril(cx.k_tall_schur(dinv)))
    return out


@functools.lru_cache(maxsize=None)
def _fresh_kernel_outputs(name):
    form = FORMS[name]
    fam = family(form.family)
    cx = _context(form)
    form.upload(cx, fam, "good")
    out = _kernel_outputs(cx, form, fam, check=True)
    cx.close()
    return out


@pytest.mark.parametrize("route", ["overrun", "nan", "zero", "limit"])
@pytest.mark.parametrize("name", [k for k in SINGLES if not FORMS[k].knobs and FORMS[k].upload is not _up_device])
def test_kernel_entries_on_a_dirtied_context(built, name, route):
    form = FORMS[name]
    fam = family(form.family)
    cx = _context(form)
    form.upload(cx, fam, "good")
    _dirty(cx, form, fam, route)
    got, want = _kernel_outputs(cx, form, fam), _fresh_kernel_outputs(name)
    cx.close()
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (name, route, k)
