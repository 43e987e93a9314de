"""lpipm_set_first_factor_cache and lpipm_update_vectors without a device: declared, exported, bound with the table's
argument types, and a null context is a bad argument."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lpipm_set_first_factor_cache": [C.c_void_p, C.c_int],
       "lpipm_update_vectors": [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]}


def test_new_symbols_are_declared_exported_and_bound(built):
    from lp_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    L = _capi.lib()
    for name, argtypes in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*lpipm_ctx\s*\*", hdr), name
        assert _capi.SYMBOLS[name] == (C.c_int, argtypes)
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes


def test_null_context_is_a_bad_argument(built):
    from lp_amd import _capi
    L = _capi.lib()
    v = (C.c_double * 4)()
    assert L.lpipm_set_first_factor_cache(None, 1) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_set_first_factor_cache(None, 0) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_vectors(None, v, v) == _capi.ERR_BAD_ARGUMENT
