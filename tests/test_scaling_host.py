"""lpipm_set_scaling and lpipm_get_scaling without a device: declared, exported, bound with the table's argument types; a
null context is a bad argument, and passes of -1 and 65 are refused (on a live context too: tests/test_gpu_scaling.py)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lpipm_set_scaling": [C.c_void_p, C.c_int],
       "lpipm_get_scaling": [C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]}


def test_new_symbols_are_declared_exported_and_bound(built):
    from lp_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    L = _capi.lib()
    for name, argtypes in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*(const\s+)?lpipm_ctx\s*\*", hdr), name
        assert _capi.SYMBOLS[name] == (C.c_int, argtypes)
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\bpub fn " + name + r"\(", ffi), name


def test_null_context_is_a_bad_argument(built):
    from lp_amd import _capi
    L = _capi.lib()
    e = (C.c_int32 * 4)()
    for passes in (0, 1, 8, 64):
        assert L.lpipm_set_scaling(None, passes) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_get_scaling(None, 0, e, e) == _capi.ERR_BAD_ARGUMENT


def test_passes_out_of_range_are_refused(built):
    from lp_amd import _capi
    L = _capi.lib()
    assert L.lpipm_set_scaling(None, -1) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_set_scaling(None, 65) == _capi.ERR_BAD_ARGUMENT


def test_context_has_the_two_methods(built):
    import lp_amd
    assert callable(lp_amd.Context.set_scaling) and callable(lp_amd.Context.scaling)
