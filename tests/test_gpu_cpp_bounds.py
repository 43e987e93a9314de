"""ProblemBuilder::lower of include/ripped.hpp (the C++ host-side mirror) through tests/cpp/test_ripped_bounds.cpp: a shifted, a
reflected and a free column through lpipm_upload_bounds, the duals' and the certificate's tail slicing."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_ripped_bounds.bin")


@pytest.mark.gpu
def test_cpp_general_bounds_on_gpu(built):
    lib = os.path.join(ROOT, "lp_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_ripped_bounds.cpp"), "-o", EXE, "-L", lib, "-llpipm",
                    f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
