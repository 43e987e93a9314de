"""lpipm_upload_device, lpipm_update_vectors_device and lpipm_k_resident_matrix without a device: the symbols are declared,
exported, bound with the table's argument types and declared for Rust; the ctypes descriptor has the C struct's size and
offsets; a null context or descriptor is a bad argument; the host-only rules of the upload (lp_amd/csrc/device_source.hpp)
hold in a stand-alone program; and Context.upload_device / lp_amd.batch.solve_device refuse wrong shapes, mixed dtypes and
CPU tensors before a context is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _u64, _vp = C.POINTER(C.c_double), C.c_uint64, C.c_void_p
UPLOAD, UPDATE, IMAGE, PACK = "lpipm_upload_device", "lpipm_update_vectors_device", "lpipm_k_resident_matrix", "lpipm_k_pack_matrix"
ARGTYPES = {
    UPLOAD: [_vp, None],
    PACK: [_vp, None, C.c_int, _dp, _dp],
    UPDATE: [_vp, _vp, _vp],
    IMAGE: [_vp, _u64, _u64, _u64, _dp, _u64, C.POINTER(_u64), C.POINTER(_u64)],
}


@pytest.mark.parametrize("name", [UPLOAD, UPDATE, IMAGE, PACK])
def test_the_symbol_is_declared_exported_and_bound(built, name):
    from lp_amd import _capi
    want = [C.POINTER(_capi.DeviceProblem) if t is None else t for t in ARGTYPES[name]]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpipm.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*lpipm_ctx\s*\*", hdr)
    assert re.search(r"\bpub fn " + name + r"\s*\(", ffi)
    assert _capi.SYMBOLS[name] == (C.c_int, want)
    fn = getattr(_capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == want


def test_rust_declares_the_structs_as_repr_c():
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ("lpipm_dev_matrix", "lpipm_dev_vector", "lpipm_device_problem"):
        assert re.search(r"#\[repr\(C\)\]\s*(#\[derive\([^)]*\)\]\s*)?pub struct " + name + r"\b", ffi), name


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "lpipm.h"
#define F(s, f) printf(#s "." #f " %zu\n", offsetof(s, f))
int main(void) {
    printf("lpipm_dev_matrix %zu\nlpipm_dev_vector %zu\nlpipm_device_problem %zu\n", sizeof(lpipm_dev_matrix),
           sizeof(lpipm_dev_vector), sizeof(lpipm_device_problem));
    F(lpipm_dev_matrix, ptr); F(lpipm_dev_matrix, row_stride); F(lpipm_dev_matrix, col_stride); F(lpipm_dev_matrix, member_stride);
    F(lpipm_dev_vector, ptr); F(lpipm_dev_vector, stride); F(lpipm_dev_vector, member_stride);
    F(lpipm_device_problem, struct_size); F(lpipm_device_problem, form); F(lpipm_device_problem, src_type);
    F(lpipm_device_problem, shared); F(lpipm_device_problem, count); F(lpipm_device_problem, m); F(lpipm_device_problem, m_eq);
    F(lpipm_device_problem, n); F(lpipm_device_problem, n_slack); F(lpipm_device_problem, A); F(lpipm_device_problem, A_eq);
    F(lpipm_device_problem, b); F(lpipm_device_problem, c); F(lpipm_device_problem, c0);
    printf("enums %d %d %d %d %d\n", LPIPM_FORM_SLACK, LPIPM_FORM_UB_EQ, LPIPM_FORM_UB_TALL, LPIPM_SRC_F64, LPIPM_SRC_F32);
    return 0;
}
"""


def test_the_ctypes_structs_have_the_c_layout(tmp_path):
    from lp_amd import _capi
    src, exe = tmp_path / "layout.c", tmp_path / "layout.bin"
    src.write_text(LAYOUT_C)
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {k: v for k, _, v in (ln.partition(" ") for ln in lines if ln)}
    structs = {"lpipm_dev_matrix": _capi.DevMatrix, "lpipm_dev_vector": _capi.DevVector, "lpipm_device_problem": _capi.DeviceProblem}
    fields = 0
    for key, val in got.items():
        if key == "enums":
            assert val.split() == [str(v) for v in (_capi.FORM_SLACK, _capi.FORM_UB_EQ, _capi.FORM_UB_TALL, _capi.SRC_F64, _capi.SRC_F32)]
        elif "." in key:
            s, f = key.split(".")
            assert getattr(structs[s], f).offset == int(val), key
            fields += 1
        else:
            assert C.sizeof(structs[key]) == int(val), key
    assert fields == sum(len(s._fields_) for s in structs.values())      # every field of every struct was compared


def test_null_context_and_null_descriptor_are_bad_arguments(built):
    from lp_amd import _capi
    L = _capi.lib()
    d = _capi.DeviceProblem(struct_size=C.sizeof(_capi.DeviceProblem), count=1, m=2, n=3)
    assert L.lpipm_upload_device(None, C.byref(d)) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_upload_device(None, None) == _capi.ERR_BAD_ARGUMENT
    assert L.lpipm_k_pack_matrix(None, C.byref(d), 1, None, None) == _capi.ERR_BAD_ARGUMENT
    v = (C.c_double * 4)()
    assert L.lpipm_update_vectors_device(None, C.cast(v, _vp), C.cast(v, _vp)) == _capi.ERR_BAD_ARGUMENT
    shape = (_u64 * 2)()
    assert L.lpipm_k_resident_matrix(None, 0, 1, 1, v, 1, shape, shape) == _capi.ERR_BAD_ARGUMENT


def test_descriptor_rules_in_a_host_only_program(tmp_path):
    """Descriptor -> host entry, refusals, farthest element with overflow near 2^63, copy modes: pure host code, so it runs
    under the address and undefined-behaviour sanitizers."""
    exe = tmp_path / "test_device_source.bin"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "lp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_device_source.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


class _NoDevice:
    """Stands where a Context would: any use of it is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the call touched the context ({name}) before validating its inputs")


class _FakeCuda:
    """What _device_request reads of a CUDA tensor, without a device: a CPU tensor that says it is on cuda:0."""
    def __new__(cls, t):
        import torch

        class T(torch.Tensor):
            is_cuda = True
            device = torch.device("cuda", 0)
        return t.as_subclass(T)


def _cases():
    import torch
    f64 = lambda *s: _FakeCuda(torch.ones(*s, dtype=torch.float64))
    f32 = lambda *s: _FakeCuda(torch.ones(*s, dtype=torch.float32))
    import lp_amd
    dims, val = lp_amd.IncompatibleInputDimensions, ValueError
    return [
        # (A, b, c, keywords, what is raised)
        (f64(5, 7), f64(4), f64(7), {}, dims),                        # b too short
        (f64(5, 7), f64(5), f64(6), {}, dims),                        # c too short
        (f64(5, 7), f64(3, 5), f64(2, 7), {}, dims),                  # shared: b and c disagree about the count
        (f64(3, 5, 7), f64(5), f64(7), {}, dims),                     # own matrices need [K, .] vectors
        (f64(3, 5, 7), f64(2, 5), f64(3, 7), {}, dims),
        (f64(2, 3, 5, 7), f64(3, 5), f64(3, 7), {}, dims),            # a 4-D A
        (f64(7), f64(5), f64(7), {}, dims),                           # a 1-D A
        (f64(5, 7), f64(5), f64(7), {"c0s": [0.0, 1.0]}, dims),       # c0 per member
        (f64(5, 7), f64(3, 8), f64(3, 7), {"form": "ub_eq", "A_eq": f64(2, 7)}, dims),        # b is [b_ub; b_eq]: 7 entries
        (f64(5, 7), f64(3, 7), f64(3, 7), {"form": "ub_eq", "A_eq": f64(2, 6)}, dims),        # A_eq has other columns
        (f64(5, 7), f64(5), f64(7), {"form": "ub_tall", "A_eq": f64(2, 7)}, val),             # tall has no eq rows
        (f64(5, 7), f64(5), f64(7), {"form": "ub_tall", "n_slack": 2}, val),                  # the hint is the slack form's
        (f64(5, 7), f64(5), f64(7), {"form": "dense"}, val),
        (f64(5, 7), f32(5), f64(7), {}, val),                         # mixed dtypes
        (f32(5, 7), f32(5), f64(7), {}, val),
        (_FakeCuda(torch.ones(5, 7, dtype=torch.float16)), _FakeCuda(torch.ones(5, dtype=torch.float16)),
         _FakeCuda(torch.ones(7, dtype=torch.float16)), {}, val),     # neither float64 nor float32
        (torch.ones(5, 7, dtype=torch.float64), f64(5), f64(7), {}, val),                     # a CPU tensor in each place
        (f64(5, 7), torch.ones(5, dtype=torch.float64), f64(7), {}, val),
        (f64(5, 7), f64(5), torch.ones(7, dtype=torch.float64), {}, val),
        (np.ones((5, 7)), np.ones(5), np.ones(7), {}, val),           # host arrays go through the upload* methods
    ]


def test_upload_device_refuses_bad_inputs_before_touching_a_context():
    import lp_amd
    for A, b, c, kw, exc in _cases():
        kw = dict(kw)
        c0s = kw.pop("c0s", None)
        with pytest.raises(exc):
            lp_amd.Context.upload_device(_NoDevice(), A, b, c, c0s, **kw)


def test_solve_device_refuses_bad_inputs_before_touching_a_context():
    import torch
    from lp_amd import batch
    import lp_amd
    for A, b, c, kw, exc in _cases():
        kw = dict(kw)
        c0s = kw.pop("c0s", None)
        with pytest.raises(exc):
            batch.solve_device(A, b, c, c0s, ctx=_NoDevice(), **kw)
    one = lambda *s: _FakeCuda(torch.ones(*s, dtype=torch.float64))
    with pytest.raises(lp_amd.IncompatibleInputDimensions):                # a single LP is not a batch
        batch.solve_device(one(5, 7), one(5), one(7), ctx=_NoDevice())
    with pytest.raises(lp_amd.InvalidParameter):
        batch.solve_device(one(5, 7), one(2, 5), one(2, 7), ctx=_NoDevice(), max_group=0)
