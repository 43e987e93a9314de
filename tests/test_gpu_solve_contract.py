"""The solve contract on a device: every case of tests/golden/make_solve_contract.py replayed on the code under test -- the
single, lockstep and batch solve entries over the recorded problems, settings and destinations, and every argument error -- must
give the recorded return code and, per member, the recorded status, iteration count and hashes of fun and x
(tests/golden/solve_contract.json)."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def load_contract():
    spec = importlib.util.spec_from_file_location("make_solve_contract", os.path.join(HERE, "golden", "make_solve_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.load()


def test_every_solve_keeps_its_return_code_and_results(built):
    from lp_amd import _capi
    mod, rec = load_contract()
    cus = mod.cu_count()
    assert cus == rec["cu_count"], (
        f"solve_contract.json was recorded on a device of {rec['cu_count']} CUs and this one has {cus}: the kernels' plans, and "
        "with them the bits of a solve, depend on the count -- record it on this device with tests/golden/make_solve_contract.py "
        "at a commit whose results are the intended ones")
    got = mod.device_cases(_capi.lib())
    assert sorted(got) == sorted(rec["device"])
    wrong = {k: (got[k], rec["device"][k]) for k in got if got[k] != rec["device"][k]}
    assert not wrong, f"{len(wrong)} of {len(got)} cases differ (got, recorded): {dict(list(wrong.items())[:4])}"
