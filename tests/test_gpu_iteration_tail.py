"""The tail of an iteration in every form it takes: every case of tests/golden/make_iteration_tail.py replayed on the code under
test -- whole solves of the dense form (kept first factor, refinement, both QR arms, the unfused vector stage by knob and by
size, the predictor beside the chain), of the tall forms and of every batch form, a column split over two ranks, one
lpipm_k_iteration per form from a seeded iterate, lpipm_k_tall_sym_solve, a tall LP with more equality rows than columns and the
counters of a profiled solve -- must give what was recorded on the parent of the commit that made the tail one sequence of named
steps (tests/golden/iteration_tail_parent.json): return codes, statuses, iteration counts and the hashes of every result."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_every_form_of_the_tail_computes_what_the_parent_computed(built, monkeypatch):
    monkeypatch.syspath_prepend(GOLDEN)              # (by name: the column split's ranks are spawned from the module)
    import make_iteration_tail as mod
    rec = mod.load()
    cus = mod.cu_count()
    assert cus == rec["cu_count"], (
        f"iteration_tail_parent.json was recorded on a device of {rec['cu_count']} CUs and this one has {cus}: the kernels' plans, "
        "and with them the bits of a solve, depend on the count -- record it on this device with "
        "tests/golden/make_iteration_tail.py at a commit whose results are the intended ones")
    got = mod.cases(monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    got = {k: json.loads(json.dumps(v)) for k, v in got.items()}
    assert sorted(got) == sorted(rec["cases"])
    wrong = {k: (got[k], rec["cases"][k]) for k in got if got[k] != rec["cases"][k]}
    assert not wrong, f"{len(wrong)} of {len(got)} cases differ (got, recorded): {dict(list(wrong.items())[:3])}"
    sys.modules.pop("make_iteration_tail", None)
