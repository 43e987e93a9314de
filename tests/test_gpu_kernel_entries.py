"""The kernel-granularity entries (Context.k_* over lpipm_k_*): every case of tests/golden/make_kernel_entries.py replayed on
the code under test -- the stand-alone factor entries at m = 1, 128, 200 and 600 with 1 and 2 right-hand sides, 1 and 3 repeats
and three splits, a matrix whose last pivot is negative, the refusals after a QR factorisation and at a size never factored,
the lockstep factorisation and substitution, the entries on a dense, a slack-hinted, a `ub`+`eq`, a scaled and both tall
resident problems, the tall entries' refusals, the pack launch on both device uploads and every entry on a context with nothing
resident -- must give what was recorded on the parent of the commit that gave the entries one timer, one padded copy and owned
scratch buffers (tests/golden/kernel_entries_parent.json): exception classes, integers and the hashes of every array.

Then the wrappers' shape checks: an array one element short or of a wrong number of dimensions is IncompatibleInputDimensions
before any C entry sees it, and the next well-formed calls on the same context return what the record says."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mod(built):
    sys.path.insert(0, GOLDEN)
    import make_kernel_entries as m
    yield m
    sys.path.remove(GOLDEN)
    sys.modules.pop("make_kernel_entries", None)


@pytest.fixture(scope="module")
def record(mod):
    rec = mod.load()
    cus = mod.cu_count()
    assert cus == rec["cu_count"], (
        f"kernel_entries_parent.json was recorded on a device of {rec['cu_count']} CUs and this one has {cus}: the kernels' plans, "
        "and with them the bits of a solve, depend on the count -- record it on this device with "
        "tests/golden/make_kernel_entries.py at a commit whose results are the intended ones")
    return rec["cases"]


def test_every_entry_returns_what_the_parent_returned(mod, record):
    got = mod.leaves(mod.cases())
    assert sorted(got) == sorted(record)
    wrong = {k: (got[k], record[k]) for k in got if got[k] != record[k]}
    assert not wrong, f"{len(wrong)} of {len(got)} records differ (got, recorded): {dict(list(wrong.items())[:3])}"


# ---- the shape checks -----------------------------------------------------------------------------------------------------------------
class _Spy:
    """The library with the name of every function called through it noted."""
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return f(*args)
        return call


@pytest.fixture
def refused(monkeypatch):
    """refused(call): `call` raises IncompatibleInputDimensions and reaches no kernel entry on the way, but for the question
    whether a problem is resident (lpipm_k_resident_matrix with no buffer)."""
    import lp_amd
    from lp_amd import _capi
    spy = _Spy(_capi.lib())
    monkeypatch.setattr(_capi, "lib", lambda: spy)

    def check(call):
        del spy.calls[:]
        with pytest.raises(lp_amd.IncompatibleInputDimensions):
            call()
        assert [f for f in spy.calls if f.startswith("lpipm_k_") and f != "lpipm_k_resident_matrix"] == [], spy.calls
    return check


def _recorded(mod, record, label, rec):
    got = mod.leaves(json.loads(json.dumps(rec)), "/" + label)
    assert got and got == {k: record.get(k) for k in got}


def test_a_resident_entry_refuses_a_short_or_misshapen_array_and_then_works(mod, record, refused):
    def body(ctx):
        m, n = ctx.m, ctx.n
        assert (m, n) == (70, 150)
        one_n, one_m = np.ones(n), np.ones(m)
        refused(lambda: ctx.k_adat(np.ones(n - 1)))
        refused(lambda: ctx.k_adat(np.ones((1, n))))
        for k, length in ((ctx.k_gemv_n, n), (ctx.k_gemv_t, m)):
            refused(lambda: k(np.ones(length - 1)))
            refused(lambda: k(np.ones(2 * length - 1)))
            refused(lambda: k(np.ones((2, length - 1))))
            refused(lambda: k(np.ones((3, length))))
            refused(lambda: k(np.ones((1, 2, length))))
        refused(lambda: ctx.k_gemv_dual(np.ones(n - 1), one_m))
        refused(lambda: ctx.k_gemv_dual(one_n, np.ones(m - 1)))
        refused(lambda: ctx.k_gemv_dual(np.ones((1, n)), one_m))
        refused(lambda: ctx.k_gemv_dual(one_n, np.ones((1, m))))
        for x, y, z in ((np.ones(n - 1), one_m, one_n), (one_n, np.ones(m - 1), one_n), (one_n, one_m, np.ones(n - 1)),
                        (np.ones((1, n)), one_m, one_n), (one_n, np.ones((1, m)), one_n), (one_n, one_m, np.ones((1, n)))):
            refused(lambda: ctx.k_iteration(mod.opts(), x, y, z, 1.0, 1.0))
        _recorded(mod, record, "resident:dense:70x150", mod.resident(ctx))
    mod.on_context(body, mod.up_dense)


def test_a_factor_entry_refuses_a_short_or_misshapen_array_and_then_works(mod, record, refused):
    m = 200
    M = mod.spd(1, m)

    def body(ctx):
        for k in (ctx.k_potrf, lambda A: ctx.k_qr_solve(A, np.ones(m)), lambda A: ctx.k_symv_residual(A, np.ones(m), np.ones(m))):
            refused(lambda: k(M.ravel()[:-1]))
            refused(lambda: k(M[:, :-1]))
            refused(lambda: k(M[None]))
        for k in (lambda R: ctx.k_chol_solve(m, R), lambda R: ctx.k_chol_solve_split(m, R, 1), lambda R: ctx.k_qr_solve(M, R),
                  lambda R: ctx.k_symv_residual(M, R, np.ones(R.shape)), lambda R: ctx.k_symv_residual(M, np.ones(R.shape), R)):
            refused(lambda: k(np.ones(m - 1)))
            refused(lambda: k(np.ones(2 * m - 1)))
            refused(lambda: k(np.ones((2, m - 1))))
            refused(lambda: k(np.ones((3, m))))
            refused(lambda: k(np.ones((1, 2, m))))
        refused(lambda: ctx.k_symv_residual(M, np.ones((1, m)), np.ones((2, m))))      # V and R0 alike
        refused(lambda: ctx.k_symv_residual(M, np.ones((2, m)), np.ones(m)))
        _recorded(mod, record, f"factor:{m}", mod.factor(ctx, m))
    mod.on_context(body)


def test_the_lockstep_factorisation_refuses_misshapen_members_and_then_works(mod, record, refused):
    def body(ctx):
        Ms = mod.lockstep_matrices(100, 1, None)
        refused(lambda: ctx.k_potrf_lockstep(Ms[0]))
        refused(lambda: ctx.k_potrf_lockstep(Ms.ravel()[:-1]))
        refused(lambda: ctx.k_potrf_lockstep(Ms[:, :, :-1]))
        refused(lambda: ctx.k_potrf_lockstep(Ms[None]))
        _recorded(mod, record, "potrf_lockstep:100x1", mod.potrf_lockstep(ctx, 100, 1))
    mod.on_context(body)
