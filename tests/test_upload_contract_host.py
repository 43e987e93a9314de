"""The upload contract without a device: every error case of tests/golden/make_upload_contract.py made with a null context
returns what tests/golden/upload_contract.json records -- among them the pairs that show which of two conditions wins (a null
context with m == 0, with count == 0, with a null matrix of no rows)."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def load_contract():
    spec = importlib.util.spec_from_file_location("make_upload_contract", os.path.join(HERE, "golden", "make_upload_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.OUT) as f:
        return mod, json.load(f)


def test_null_context_return_codes(built):
    from lp_amd import _capi
    mod, rec = load_contract()
    got = mod.host_cases(_capi.lib())
    assert sorted(got) == sorted(rec["host"])
    wrong = {k: (got[k], rec["host"][k]) for k in got if got[k] != rec["host"][k]}
    assert not wrong, f"(got, recorded): {wrong}"
    assert _capi.UNCONSTRAINED in got.values() and _capi.ERR_BAD_ARGUMENT in got.values()
