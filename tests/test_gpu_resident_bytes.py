"""The layouts of every resident form, pinned: each upload of tests/golden/make_resident_bytes.py, with the first-factor cache
on and off, must leave exactly the bytes recorded in tests/golden/resident_bytes_parent.json -- taken before each normal
system's matrix, plan and launch became one value, which must not move a single take.  Allocations only; nothing is solved."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_form_keeps_its_resident_bytes(built):
    spec = importlib.util.spec_from_file_location("make_resident_bytes", os.path.join(HERE, "golden", "make_resident_bytes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.OUT) as f:
        rec = json.load(f)
    cus = mod.cu_count()
    assert cus == rec["cu_count"], (
        f"resident_bytes_parent.json was recorded on a device of {rec['cu_count']} CUs and this one has {cus}: the A.D.A^T "
        "plan, and with it the arena's slabs, depends on the count")
    got = mod.measure()
    assert sorted(got) == sorted(rec["bytes"]) and len(got) == 22
    wrong = {k: (got[k], rec["bytes"][k]) for k in got if got[k] != rec["bytes"][k]}
    assert not wrong, f"{len(wrong)} of {len(got)} uploads differ (got, recorded): {wrong}"
