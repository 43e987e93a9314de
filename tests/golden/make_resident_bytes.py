"""Records how many bytes every resident form leaves on the device.

resident_bytes_parent.json : Context.resident_bytes() after each upload of cases(), with the first-factor cache on and off,
                             plus the CU count of the device it was recorded on (the A.D.A^T plan, and with it the slabs of
                             an arena, depends on it).  tests/test_gpu_resident_bytes.py makes the same uploads on the code
                             under test and requires equality: a change of the layouts -- the order of the takes in an
                             arena or in the shared allocation, a buffer more or less -- shows here.

The record is the layout of the commit it was taken at (the parent of the one that gathered each normal system's matrix,
plan and launch into one value): regenerate it only at a commit whose layout is the intended one, never to make a failing
comparison pass.  Only the public Python API is used, so the script runs unchanged at any commit that has it.
Run from the repo root on an MI355X:  python tests/golden/make_resident_bytes.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "resident_bytes_parent.json")


def _slack(rng, m, nx):
    """m x (nx + m): structural columns, then the slack block I."""
    return np.hstack([rng.standard_normal((m, nx)), np.eye(m)])


def cases():
    """(label, upload): upload(ctx) makes the form resident.  Only the shapes matter; the numbers are never solved."""
    import lp_amd
    rng = np.random.default_rng(0)
    K = 3
    vecs = lambda k: [rng.standard_normal(k) for _ in range(K)]
    A = rng.standard_normal((200, 300))
    As = _slack(rng, 200, 100)
    A_ub, A_eq = rng.standard_normal((150, 90)), rng.standard_normal((20, 90))
    X, E = rng.standard_normal((600, 40)), rng.standard_normal((5, 40))
    parts = lp_amd.Problem.target(rng.standard_normal(90)).ub(A_ub, rng.standard_normal(150)).eq(A_eq, rng.standard_normal(20)).build()
    tall = lp_amd.Problem.target(rng.standard_normal(40)).ub(X, rng.standard_normal(600)).build()
    tall_eq = lp_amd.Problem.target(rng.standard_normal(40)).ub(X, rng.standard_normal(600)).eq(E, rng.standard_normal(5)).build()
    return [
        ("dense:200x300", lambda c: c.upload_arrays(A, rng.standard_normal(200), rng.standard_normal(300))),
        ("dense_hint:200x300", lambda c: c.upload_arrays(As, rng.standard_normal(200), rng.standard_normal(300), n_slack=200)),
        ("ub_eq:150+20x90", lambda c: c.upload(parts)),
        ("lockstep:3x200x300", lambda c: c.upload_lockstep([A, A + 1.0, A - 1.0], vecs(200), vecs(300))),
        ("shared:3x200x300", lambda c: c.upload_lockstep_shared(A, vecs(200), vecs(300))),
        ("shared_ub_eq:3x150+20x90", lambda c: c.upload_lockstep_shared_ub_eq(A_ub, A_eq, vecs(170), vecs(90))),
        ("tall:600x40", lambda c: c.upload(tall, tall=True)),
        ("tall_eq:600x40+5", lambda c: c.upload_tall_eq(tall_eq)),
        ("shared_tall:3x600x40", lambda c: c.upload_lockstep_shared_ub_tall(X, vecs(600), vecs(40))),
        ("shared_tall_eq:3x600x40+5", lambda c: c.upload_lockstep_shared_ub_eq_tall(X, E, vecs(605), vecs(40))),
        ("owned_tall:3x600x40", lambda c: c.upload_lockstep_ub_tall([X, X + 1.0, X - 1.0], vecs(600), vecs(40))),
    ]


def measure():
    """-> {"<label>:cache<0|1>": bytes}, each upload on a context of its own."""
    import lp_amd
    rec = {}
    for label, upload in cases():
        for cache in (1, 0):
            ctx = lp_amd.Context(0)
            ctx.set_first_factor_cache(bool(cache))
            upload(ctx)
            rec[f"{label}:cache{cache}"] = ctx.resident_bytes()
            ctx.close()
    return rec


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def main():
    doc = dict(note="recorded by tests/golden/make_resident_bytes.py; bytes: label -> Context.resident_bytes()",
               cu_count=cu_count(), bytes=measure())
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(doc["bytes"]), "uploads, CU count", doc["cu_count"])


if __name__ == "__main__":
    main()
