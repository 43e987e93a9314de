"""The solve contract without a device.  Every argument error of tests/golden/make_solve_contract.py made with a null context
returns what tests/golden/solve_contract.json records and leaves every output as it was; and the steps that divide a batch into
lockstep chunks and a rest (lp_amd/csrc/batch_plan.hpp: no device, no HIP call) follow their rules in a host-only program."""
import importlib.util
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def load_contract():
    spec = importlib.util.spec_from_file_location("make_solve_contract", os.path.join(HERE, "golden", "make_solve_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.load()


def test_null_context_return_codes_and_untouched_outputs(built):
    from lp_amd import _capi
    mod, rec = load_contract()
    got = mod.host_cases(_capi.lib())
    assert sorted(got) == sorted(rec["host"])
    wrong = {k: (got[k], rec["host"][k]) for k in got if got[k] != rec["host"][k]}
    assert not wrong, f"(got, recorded): {wrong}"
    assert {r["rc"] for r in got.values()} == {_capi.ERR_BAD_ARGUMENT}


def test_batch_plan_rules():
    exe = os.path.join(ROOT, "tests", "cpp", "test_batch_plan.bin")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "lp_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_batch_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
