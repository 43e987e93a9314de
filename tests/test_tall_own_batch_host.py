"""lpipm_upload_lockstep_ub_tall and lpipm_solve_batch_ub_tall without a device: both symbols are declared, exported, bound
with the table's argument types and declared for Rust, a null context is a bad argument, and Context.solve_batch(...,
tall=True) / solve_batch_device / lp_amd.batch.solve_batch_sharded refuse a Problem with `eq` rows before a context is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u64 = C.POINTER(C.c_double), C.c_uint64
_dpp, _u64p = C.POINTER(_dp), C.POINTER(C.c_uint64)
UPLOAD, BATCH = "lpipm_upload_lockstep_ub_tall", "lpipm_solve_batch_ub_tall"
ARGTYPES = {
    UPLOAD: [C.c_void_p, _u64, _u64, _u64, _dpp, _u64, _dpp, _dpp, _dp],
    BATCH: [C.c_void_p, _u64, _u64p, _u64p, _dpp, _dpp, _dpp, _dp, None, _dpp, C.c_void_p, _u64, _dp, _u64p, C.POINTER(C.c_int32)],
}


@pytest.mark.parametrize("name", [UPLOAD, BATCH])
def test_the_symbol_is_declared_exported_and_bound(built, name):
    from lp_amd import _capi
    want = [C.POINTER(_capi.Opts) if t is None else t for t in ARGTYPES[name]]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*lpipm_ctx\s*\*", hdr)
    assert re.search(r"\bpub fn " + name + r"\s*\(", ffi)
    assert _capi.SYMBOLS[name] == (C.c_int, want)
    fn = getattr(_capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == want


def test_null_context_is_a_bad_argument(built):
    from lp_amd import _capi
    L = _capi.lib()
    X, v = (C.c_double * 6)(), (C.c_double * 5)()
    rows, mats = (_dp * 1)(C.cast(v, _dp)), (_dp * 1)(C.cast(X, _dp))
    up = getattr(L, UPLOAD)
    assert up(None, 1, 2, 3, mats, 2, rows, rows, None) == _capi.ERR_BAD_ARGUMENT
    assert up(None, 1, 2, 0, None, 2, rows, rows, None) == _capi.ERR_BAD_ARGUMENT
    opts = _capi.Opts()
    L.lpipm_default_opts(C.byref(opts))
    m, n = (_u64 * 1)(3), (_u64 * 1)(2)
    st = (C.c_int32 * 1)()
    assert getattr(L, BATCH)(None, 1, m, n, mats, rows, rows, None, C.byref(opts), rows, None, 0, None, None, st) == _capi.ERR_BAD_ARGUMENT


class _NoDevice:
    """Stands where a Context would: any use of it is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the call touched the context ({name}) before validating its inputs")


def _problems():
    import lp_amd
    X = np.ones((5, 2))
    pure = lp_amd.Problem.target(np.ones(2)).ub(X, np.ones(5)).build()
    with_eq = lp_amd.Problem.target(np.ones(2)).ub(X, np.ones(5)).eq(np.ones((1, 2)), np.ones(1)).build()
    return pure, with_eq


def test_solve_batch_tall_refuses_eq_rows_before_touching_a_context():
    import lp_amd
    pure, with_eq = _problems()
    opts = lp_amd.InteriorPoint.default().opts()
    with pytest.raises(ValueError):
        lp_amd.Context.solve_batch(_NoDevice(), [pure, with_eq], opts, tall=True)
    with pytest.raises(ValueError):
        lp_amd.Context.solve_batch_device(_NoDevice(), [with_eq], opts, 0, 16, tall=True)
    with pytest.raises(ValueError):                                  # members in the (A, b, c, c0) form are no Problems
        lp_amd.Context.solve_batch(_NoDevice(), [(np.ones((5, 2)), np.ones(5), np.ones(2), 0.0)], opts, tall=True)


def test_solve_batch_sharded_passes_the_flag_through():
    from lp_amd import batch
    pure, with_eq = _problems()
    with pytest.raises(ValueError):
        batch.solve_batch_sharded([pure, with_eq], ctx=_NoDevice(), tall=True)
