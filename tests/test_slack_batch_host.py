"""Host-side view of the slack-batch entry points (no GPU): declared in include/lpipm.h, exported by liblpipm.so, bound by
lp_amd._capi, and refusing a null context before anything touches a device."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lpipm_upload_lockstep_slack", "lpipm_upload_lockstep_shared_slack", "lpipm_upload_lockstep_shared_ub_eq",
       "lpipm_solve_batch_slack")


def test_symbols_declared_and_resolved(built):
    from lp_amd import _capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lpipm_[a-z0-9_]+)\s*\(", hdr))
    L = _capi.lib()
    for name in NEW:
        assert name in declared and name in _capi.SYMBOLS, name
        assert getattr(L, name).argtypes == _capi.SYMBOLS[name][1], name


def test_null_context_is_a_bad_argument(built):
    from lp_amd import _capi
    L = _capi.lib()
    dp = C.POINTER(C.c_double)
    K, m, n = 2, 2, 3
    A = np.array([[1.0, 1.0, 1.0], [1.0, 2.0, 0.0]])
    bs = [np.ones(m) for _ in range(K)]; cs = [np.ones(n) for _ in range(K)]; cx = [np.ones(2) for _ in range(K)]
    arr = lambda lst: (dp * len(lst))(*[x.ctypes.data_as(dp) for x in lst])
    pa = A.ctypes.data_as(dp)
    BAD = _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_upload_lockstep_slack(None, K, m, n, arr([A] * K), arr(bs), arr(cs), None, 1) == BAD
    assert L.lpipm_upload_lockstep_shared_slack(None, K, m, n, pa, n, arr(bs), arr(cs), None, 1) == BAD
    assert L.lpipm_upload_lockstep_shared_ub_eq(None, K, 2, 1, pa, n, 1, pa, n, arr(bs), arr(cx), None) == BAD
    o = _capi.Opts()
    L.lpipm_default_opts(C.byref(o))
    u64 = lambda v: (C.c_uint64 * K)(*v)
    xs = [np.zeros(n) for _ in range(K)]
    st = (C.c_int32 * K)()
    assert L.lpipm_solve_batch_slack(None, K, u64([m] * K), u64([n] * K), u64([1] * K), arr([A] * K), arr(bs), arr(cs), None,
                                     C.byref(o), arr(xs), None, 0, None, None, st) == BAD
