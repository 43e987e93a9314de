"""lpipm_update_lockstep_vectors[_device] and the sweep drivers' chunking without a device: the symbols are declared, exported
and bound with the table's argument types, a null context is a bad argument, and the chunks of a sweep are equal."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
NEW = {"lpipm_update_lockstep_vectors": [C.c_void_p, C.c_uint64, C.POINTER(_dp), C.POINTER(_dp), _dp],
       "lpipm_update_lockstep_vectors_device": [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _dp]}


def test_new_symbols_are_declared_exported_and_bound(built):
    from lp_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    L = _capi.lib()
    for name, argtypes in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*lpipm_ctx\s*\*", hdr), name
        assert re.search(r"\bpub fn " + name + r"\s*\(", ffi), name
        assert _capi.SYMBOLS[name] == (C.c_int, argtypes)
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes


def test_null_context_is_a_bad_argument(built):
    from lp_amd import _capi
    L = _capi.lib()
    v = (C.c_double * 4)()
    rows = (_dp * 1)(C.cast(v, _dp))
    assert L.lpipm_update_lockstep_vectors(None, 1, rows, rows, v) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_lockstep_vectors(None, 1, None, None, None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_update_lockstep_vectors_device(None, 1, None, 4, None, 4, v) == _capi.ERR_BAD_ARGUMENT


def test_sweep_chunks_are_equal_and_cover_every_member_once_in_order():
    from lp_amd.batch import sweep_chunks
    for max_group in (1, 2, 3, 4, 7, 8, 32):
        for count in range(1, 4 * max_group + 6):
            g, chunks = sweep_chunks(count, max_group)
            k = len(chunks)
            assert k == -(-count // max_group) and g == -(-count // k) and 1 <= g <= max_group
            assert all(len(ch) == g for ch in chunks), (count, max_group)
            assert k * g - count <= k - 1, (count, max_group)
            flat = [i for ch in chunks for i in ch]
            assert flat[:count] == list(range(count))                      # every member once, in order ...
            assert all(i == count - 1 for i in flat[count:])               # ... then repeats of the last one only
            assert all(i in chunks[-1] for i in flat[count:])
    assert sweep_chunks(0, 4) == (0, [])
