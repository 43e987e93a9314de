"""Wall clock of an upload, copy-in and synchronisation included: upload_lockstep of 32 x 1024x2048 and upload_arrays of
4096x8192, each two warm-ups and ten timed uploads on one context.  Prints one JSON line {name: {median, min, max}} in ms.
For a comparison of two builds run it alternately in both trees (compare_trees.sh) -- profiles/upload_refactor.md."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lp_amd
from lp_amd import synth


def timed(upload, warm=2, reps=10):
    ts = []
    for k in range(warm + reps):
        t = time.perf_counter(); upload(); ts.append((time.perf_counter() - t) * 1e3)
    ts = ts[warm:]
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


A, bs, cs, _ = synth.planted_scenarios(0, 1024, 2048, 32)
As = [A.copy() for _ in range(32)]
A3, b3, c3, _ = synth.planted_lp(0, 4096, 8192)
ctx = lp_amd.Context(0)
out = dict(upload_lockstep_32x1024x2048=timed(lambda: ctx.upload_lockstep(As, bs, cs)))
out["upload_arrays_4096x8192"] = timed(lambda: ctx.upload_arrays(A3, b3, c3))
ctx.close()
print(json.dumps(out), flush=True)
