"""InteriorPoint::solve_with_certificate() of include/ripped.hpp (the C++ host-side mirror) through
tests/cpp/test_ripped_certificate.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_ripped_certificate.bin")


@pytest.mark.gpu
def test_cpp_solve_with_certificate_on_gpu(built):
    lib = os.path.join(ROOT, "lp_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_ripped_certificate.cpp"), "-o", EXE, "-L", lib, "-llpipm",
                    f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
