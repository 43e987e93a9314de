"""Lockstep batches of tall LPs with equality rows over one image (lpipm_upload_lockstep_shared_ub_eq_tall), without a
device: the two new symbols are declared, exported and bound with the table's argument types; the Python wrappers refuse
mismatched inputs before a context is touched; and the generator of tests/test_gpu_tall_eq_batch.py lives here with the
conditions every parity shape must meet, checked with the C oracle -- an input the oracle itself does not solve fails in this file.

The generator is planted_eq of tests/test_tall_eq_host.py restated on a GIVEN pair (X, A_eq): X has row 0 >= 0 and column
0 <= 0 (shared_X of tests/test_gpu_tall_batches.py), A_eq has column 0 = 0, so b[0] = -1 makes a member infeasible and c[0] = -1
makes it unbounded; member i has its own planted vertex with b_eq = A_eq x* and c = -X^T lam - A_eq^T nu + mu."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from test_tall_eq_host import _solve_np, make_tall_eq_solver, slack_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
UPLOAD = "lpipm_upload_lockstep_shared_ub_eq_tall"
UPLOAD_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, _dp, C.c_uint64, C.c_uint64, _dp, C.c_uint64, C.POINTER(_dp),
                   C.POINTER(_dp), _dp]
KERNEL = "lpipm_k_trsm_lt_lockstep"
KERNEL_ARGTYPES = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_uint64, _dp, _ip, _ip]

X_TOL = 1e-6
INF, UNB, LOST = "infeasible", "unbounded", "lost-pivot"
# (m_ub, nx, m_eq): the parity shapes of the GPU tests
SHAPES = [(300, 40, 1), (300, 40, 5), (300, 40, 39), (1100, 130, 17)]
BASE, LARGE = (300, 40, 5), (1100, 130, 17)
# the optimal members each shape's GPU tests use (member indices): counts up to 19 and the second set of the update test at the
# base shape, counts up to 5 at the large one, count 3 at the other two
MEMBERS = {(300, 40, 1): range(1), (300, 40, 5): range(17), (300, 40, 39): range(1), (1100, 130, 17): range(3)}
FAILING = (300, 40, 41)          # m_eq > nx: S is singular by construction, every member a NumericalProblem
# Member seeds that are passed over: on these the tall-eq ALGEBRA itself -- emulated in float64 numpy inside the oracle's loop,
# make_tall_eq_solver of tests/test_tall_eq_host.py -- ends in NumericalProblem in the oracle's last iteration, under the default
# options or under ip = 0 (K alone is singular at a vertex with fewer active `ub` rows than basic columns; its last pivots are
# rounding), while the oracle on the m x m system returns Ok.  Such a member is no parity case for any implementation of the
# form; the condition is tested below.
PASSED_OVER = {(300, 40, 5): (5, 7, 11, 12), (1100, 130, 17): (0,)}
ALGEBRA_OPTIONS = [(), (("ip", False),)]


# ---- generator --------------------------------------------------------------------------------------------------------------------
def shared_pair(seed, m, nx, me):
    """-> X (row 0 >= 0, column 0 <= 0), A_eq (column 0 = 0), both ~ N(0, 1) elsewhere."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    X[0, :] = np.abs(X[0, :]); X[:, 0] = -np.abs(X[:, 0]); X[0, 0] = 0.0
    Ae = rng.standard_normal((me, nx))
    Ae[:, 0] = 0.0
    return X, Ae


def member(X, Ae, seed):
    """planted_eq on the given pair: k = max(nx // 2, me) basic structural variables, k - me active `ub` rows, multipliers in
    [1, 2] on the active rows and the nonbasic columns, free multipliers ~ N(0, 1) on the `eq` rows.  -> b, b_eq, c, x*"""
    rng = np.random.default_rng(seed)
    (m, nx), me = X.shape, Ae.shape[0]
    k = min(nx, max(nx // 2, me))
    na = max(k - me, 0)
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:na]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, na)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    nu = rng.standard_normal(me)
    return b, Ae @ xs, -X.T @ lam - Ae.T @ nu + mu, xs


@functools.lru_cache(maxsize=None)
def pair_of(shape):
    m, nx, me = shape
    X, Ae = shared_pair(100 + m + me, m, nx, me)
    X.setflags(write=False); Ae.setflags(write=False)
    return X, Ae


@functools.lru_cache(maxsize=None)
def member_of(shape, spec):
    """spec: an int i -- member i of the shape --, INF / UNB: member 0 with b[0] = -1 / c[0] = -1, or LOST: the first seed that was
    passed over, a member on which the algebra loses a pivot.
    -> b = [b_ub; b_eq] (the lockstep form), c (the nx structural costs)"""
    X, Ae = pair_of(shape)
    i = spec if isinstance(spec, int) else 0
    i = [k for k in range(i + 1 + len(PASSED_OVER.get(shape, ()))) if k not in PASSED_OVER.get(shape, ())][i]
    if spec == LOST:
        i = PASSED_OVER[shape][0]
    b, be, c, _ = member(X, Ae, 1000 * shape[0] + 10 * shape[2] + i)
    if spec == INF:
        b[0] = -1.0              # row 0 of X is >= 0 and x >= 0
    if spec == UNB:
        c[0] = -1.0              # column 0 of X is <= 0 and column 0 of A_eq is 0
    bb = np.concatenate([b, be])
    bb.setflags(write=False); c.setflags(write=False)
    return bb, c


def specs_of(count, first=0):
    """The members of a batch of `count`: optimal members first, first + 1, ...; from count 3 on the infeasible member at
    position 1 and the unbounded one last (in a batch of 19: one in each half)."""
    if count < 3:
        return list(range(first, first + count))
    return [first, INF] + list(range(first + 1, first + count - 2)) + [UNB]


def vectors_of(shape, specs):
    ms = [member_of(shape, s) for s in specs]
    return [v[0] for v in ms], [v[1] for v in ms]


def permuted_pair(X, Ae, c, seed):
    """The same LP with its structural columns permuted: -> X', A_eq', c', perm (x' = x[perm])."""
    perm = np.random.default_rng(7000 + seed).permutation(X.shape[1])
    return X[:, perm], Ae[:, perm], c[perm], perm


@functools.lru_cache(maxsize=None)
def oracle_pair(shape, spec):
    """The C oracle on the slack form of the member as generated and with its structural columns permuted (x mapped back):
    computed once, shared, never written to."""
    from oracle import capi as oracle
    m, nx, me = shape
    X, Ae = pair_of(shape)
    bb, c = member_of(shape, spec)
    b, be = bb[:m], bb[m:]
    ref = oracle.solve(*slack_form(X, b, Ae, be, c), want_log=False)
    Xp, Aep, cp, perm = permuted_pair(X, Ae, c, m + (spec if isinstance(spec, int) else 0))
    alt = oracle.solve(*slack_form(Xp, b, Aep, be, cp), want_log=False)
    if alt["x_slack"] is not None:
        back = alt["x_slack"].copy()
        back[perm] = alt["x_slack"][:nx]
        alt["x_slack"] = back
    for r in (ref, alt):
        if r["x_slack"] is not None:
            r["x_slack"].setflags(write=False)
    return ref, alt


# ---- the conditions on the generator ----------------------------------------------------------------------------------------------
def test_the_shared_pair_has_the_sign_structure():
    for shape in SHAPES + [FAILING]:
        X, Ae = pair_of(shape)
        assert (X[0, :] >= 0).all() and (X[:, 0] <= 0).all() and (Ae[:, 0] == 0).all()
        assert X.shape == shape[:2] and Ae.shape == (shape[2], shape[1])


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{nx}+{me}" for m, nx, me in SHAPES])
def test_parity_members_are_ones_the_oracle_solves(built, shape):
    """Conditions, not measurements: Ok on every optimal member as generated and with permuted columns, Infeasible on the INF
    member, Unbounded on the UNB member."""
    for i in MEMBERS[shape]:
        ref, alt = oracle_pair(shape, i)
        assert ref["status"] == 0 and alt["status"] == 0, (shape, i, ref["status"], alt["status"])
        spread = np.abs(ref["x_slack"] - alt["x_slack"]).max()
        print(f"\n[measure] {shape} member {i}: {ref['iterations']} / {alt['iterations']} iterations, oracle spread under a "
              f"column permutation {spread:.3g}")
    inf, unb = oracle_pair(shape, INF), oracle_pair(shape, UNB)
    assert inf[0]["status"] == 5 and inf[1]["status"] == 5, (shape, inf[0]["status"], inf[1]["status"])
    assert unb[0]["status"] == 6 and unb[1]["status"] == 6, (shape, unb[0]["status"], unb[1]["status"])


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{m}x{nx}+{me}" for m, nx, me in SHAPES])
def test_parity_members_are_ones_the_algebra_solves(built, shape):
    """The second condition: the algebra of the form, emulated in numpy, is Ok on every optimal member under the default options
    and under ip = 0 -- under the default ones in the oracle's iteration count, with x to X_TOL -- so a member on which the GPU
    ends elsewhere is a fault of the GPU code, not of the input."""
    m, nx, me = shape
    X, Ae = pair_of(shape)
    for i in MEMBERS[shape]:
        bb, c = member_of(shape, i)
        for kw in ALGEBRA_OPTIONS:
            got = _solve_np(*slack_form(X, bb[:m], Ae, bb[m:], c), kw, solver=make_tall_eq_solver(nx, m))
            assert got.status == 0, (shape, i, kw, got.status)
            if not kw:
                ref = oracle_pair(shape, i)[0]
                assert got.iterations == ref["iterations"], (shape, i, got.iterations, ref["iterations"])
                assert np.abs(got.x_slack - ref["x_slack"]).max() <= X_TOL, (shape, i)


def test_the_lost_pivot_member_is_one_the_algebra_does_not_solve(built):
    """The member the GPU tests use for a pivot lost in the middle of a batch: Ok for the oracle, NumericalProblem for the emulated
    algebra under the default options, in the oracle's last iteration."""
    m, nx, me = BASE
    X, Ae = pair_of(BASE)
    bb, c = member_of(BASE, LOST)
    ref = oracle_pair(BASE, LOST)[0]
    got = _solve_np(*slack_form(X, bb[:m], Ae, bb[m:], c), solver=make_tall_eq_solver(nx, m))
    assert ref["status"] == 0 and got.status == 2 and got.iterations == ref["iterations"], (ref["status"], got.status, got.iterations)


def test_more_equality_rows_than_columns_is_a_numerical_problem_for_the_oracle(built):
    from oracle import capi as oracle
    m, nx, me = FAILING
    X, Ae = pair_of(FAILING)
    for i in range(3):
        bb, c = member_of(FAILING, i)
        assert oracle.solve(*slack_form(X, bb[:m], Ae, bb[m:], c), want_log=False)["status"] == 2


# ---- the symbols ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,argtypes,rust", [(UPLOAD, UPLOAD_ARGTYPES, True), (KERNEL, KERNEL_ARGTYPES, False)],
                         ids=["upload", "kernel-entry"])
def test_the_symbols_are_declared_exported_and_bound(built, name, argtypes, rust):
    from lp_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*lpipm_ctx\s*\*", hdr)
    if rust:
        ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
        assert re.search(r"\bpub fn " + name + r"\s*\(", ffi)
    assert _capi.SYMBOLS[name] == (C.c_int, argtypes)
    fn = getattr(_capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    assert _capi.SYMBOLS[UPLOAD][1] == _capi.SYMBOLS["lpipm_upload_lockstep_shared_ub_eq"][1]


def test_calls_without_a_context_touch_nothing(built):
    from lp_amd import _capi
    L = _capi.lib()
    X, v = (C.c_double * 6)(), (C.c_double * 3)()
    rows = (_dp * 1)(C.cast(v, _dp))
    up = getattr(L, UPLOAD)
    assert up(None, 1, 2, 3, C.cast(X, _dp), 2, 1, C.cast(X, _dp), 2, rows, rows, None) == _capi.ERR_BAD_ARGUMENT
    assert up(None, 1, 2, 3, C.cast(X, _dp), 2, 0, None, 2, rows, rows, None) == _capi.ERR_BAD_ARGUMENT     # (the pure-ub entry's answer)
    assert up(None, 1, 2, 0, None, 2, 0, None, 2, rows, rows, None) == _capi.ERR_BAD_ARGUMENT
    k = getattr(L, KERNEL)
    info = (C.c_int32 * 1)()
    assert k(None, 2, 1, 1, 2, 1, C.cast(X, _dp), C.cast(X, _dp), 2, C.cast(X, _dp), info, None) == _capi.ERR_BAD_ARGUMENT


# ---- the wrappers validate before a context is touched ----------------------------------------------------------------------------
def test_upload_wrapper_value_errors():
    import lp_amd
    cx = lp_amd.Context.__new__(lp_amd.Context)          # no device: the checks come before the library is called
    up = lp_amd.Context.upload_lockstep_shared_ub_eq_tall
    X, Ae = np.ones((5, 2)), np.ones((1, 2))
    bs, cs = [np.ones(6)] * 3, [np.ones(2)] * 3
    for bad in [(X, Ae, bs, cs[:2]), (X, Ae, [], []), (X, np.ones((1, 3)), bs, cs), (np.ones((5, 3)), Ae, bs, cs),
                (X, Ae, [np.ones(5)] * 3, cs), (X, Ae, bs, [np.ones(7)] * 3), (X, np.ones(2), bs, cs)]:
        with pytest.raises(lp_amd.IncompatibleInputDimensions):
            up(cx, *bad)
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        up(cx, X, Ae, bs, cs, c0s=[0.0, 1.0])


def test_kernel_wrapper_value_errors():
    import lp_amd
    cx = lp_amd.Context.__new__(lp_amd.Context)
    k = lp_amd.Context.k_trsm_lt_lockstep
    Ms = np.stack([np.eye(4)] * 2)
    for bad in [(np.eye(4), np.ones((1, 4))), (Ms, np.ones((3, 1, 4))), (Ms, np.ones((1, 5))), (Ms, np.ones(4)),
                (np.ones((2, 4, 3)), np.ones((1, 3)))]:
        with pytest.raises(lp_amd.IncompatibleInputDimensions):
            k(cx, *bad)
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        k(cx, Ms, np.ones((1, 4)), done_mask=[0, 1, 0])


class _NoDevice:
    """Stands where a Context would: any use of it is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the driver touched the context ({name}) before validating its inputs")


@pytest.mark.parametrize("fn", ["solve_shared_ub_eq_tall", "sweep_shared_ub_eq_tall"])
def test_drivers_validate_before_touching_a_device(fn):
    import lp_amd
    from lp_amd import batch
    f = getattr(batch, fn)
    X, Ae = np.ones((5, 2)), np.ones((1, 2))
    bs, cs = [np.ones(6)] * 3, [np.ones(2)] * 3
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        f(X, Ae, bs, cs[:2], ctx=_NoDevice())
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        f(X, Ae, bs, cs, c0s=[0.0, 1.0], ctx=_NoDevice())
    for bad in (0, -1):
        with pytest.raises(lp_amd.InvalidParameter):
            f(X, Ae, bs, cs, ctx=_NoDevice(), max_group=bad)
