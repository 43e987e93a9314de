"""The upload contract on a device: every case of tests/golden/make_upload_contract.py replayed on the code under test --
each upload entry over the recorded shapes, settings and sequences, each documented error and the pairs of simultaneous
conditions -- must give the recorded return code and the recorded resident byte count (tests/golden/upload_contract.json)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def load_contract():
    spec = importlib.util.spec_from_file_location("make_upload_contract", os.path.join(HERE, "golden", "make_upload_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.OUT) as f:
        return mod, json.load(f)


def test_every_upload_keeps_its_return_code_and_resident_bytes(built):
    from lp_amd import _capi
    mod, rec = load_contract()
    cus = mod.cu_count()
    assert cus == rec["cu_count"], (
        f"upload_contract.json was recorded on a device of {rec['cu_count']} CUs and this one has {cus}: the A.D.A^T plan, and "
        "with it the arena's slabs, depends on the count -- record it on this device with tests/golden/make_upload_contract.py "
        "at a commit whose sizes are the intended ones")
    got = mod.device_cases(_capi.lib())
    assert sorted(got) == sorted(rec["device"])
    wrong = {k: (got[k], rec["device"][k]) for k in got if got[k] != rec["device"][k]}
    assert not wrong, f"{len(wrong)} of {len(got)} cases differ (got, recorded): {dict(list(wrong.items())[:12])}"
