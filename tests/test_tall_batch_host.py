"""lpipm_upload_lockstep_shared_ub_tall and its drivers without a device: the symbol is declared, exported and bound with the
table's argument types, a null context is a bad argument, and lp_amd.batch.solve_shared_ub_tall / sweep_shared_ub_tall refuse
mismatched inputs before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
NAME = "lpipm_upload_lockstep_shared_ub_tall"
ARGTYPES = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, _dp, C.c_uint64, C.POINTER(_dp), C.POINTER(_dp), _dp]


def test_the_symbol_is_declared_exported_and_bound(built):
    from lp_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*lpipm_ctx\s*\*", hdr)
    assert re.search(r"\bpub fn " + NAME + r"\s*\(", ffi)
    assert _capi.SYMBOLS[NAME] == (C.c_int, ARGTYPES)
    fn = getattr(_capi.lib(), NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGTYPES


def test_null_context_is_a_bad_argument(built):
    from lp_amd import _capi
    X, v = (C.c_double * 6)(), (C.c_double * 3)()
    rows = (_dp * 1)(C.cast(v, _dp))
    fn = getattr(_capi.lib(), NAME)
    assert fn(None, 1, 2, 3, C.cast(X, _dp), 2, rows, rows, None) == _capi.ERR_BAD_ARGUMENT
    assert fn(None, 1, 2, 0, None, 2, rows, rows, None) == _capi.ERR_BAD_ARGUMENT


class _NoDevice:
    """Stands where a Context would: any use of it is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the driver touched the context ({name}) before validating its inputs")


@pytest.mark.parametrize("fn", ["solve_shared_ub_tall", "sweep_shared_ub_tall"])
def test_drivers_validate_before_touching_a_device(fn):
    import lp_amd
    from lp_amd import batch
    f = getattr(batch, fn)
    X = np.ones((5, 2))
    bs, cs = [np.ones(5)] * 3, [np.ones(2)] * 3
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        f(X, bs, cs[:2], ctx=_NoDevice())
    with pytest.raises(lp_amd.IncompatibleInputDimensions):
        f(X, bs, cs, c0s=[0.0, 1.0], ctx=_NoDevice())
    for bad in (0, -1):
        with pytest.raises(lp_amd.InvalidParameter):
            f(X, bs, cs, ctx=_NoDevice(), max_group=bad)
