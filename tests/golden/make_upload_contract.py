"""Records the upload contract: what every upload entry of the C ABI returns and how many bytes it leaves resident.

upload_contract.json : per case the return code of the call and lpipm_get_resident_bytes afterwards, plus the CU count of
                       the device it was recorded on (the A.D.A^T plan, and with it the slabs of an arena, depends on it).
                       tests/test_gpu_upload_contract.py replays the `device` cases on the code under test and
                       tests/test_upload_contract_host.py the `host` ones (a null context: no device is touched); both
                       require equality.

The record is the behaviour of the commit it was taken at: regenerate it only at a commit whose sizes and return codes are
the intended ones (before a change that must keep them), never to make a failing replay pass.  Only public entries are
called, so the script runs unchanged at any commit that has them.
Run from the repo root on an MI355X:  python tests/golden/make_upload_contract.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "upload_contract.json")

_dp = C.POINTER(C.c_double)


class NullAt:
    """A pointer array whose entry `index` is null."""
    def __init__(self, index):
        self.index = index


def _mat(rng, m, n, slack=0, broken=False):
    """m x n; slack > 0: the last `slack` columns are [I; 0] (broken: except for one entry)."""
    A = rng.standard_normal((m, n))
    if slack:
        A[:, n - slack:] = np.eye(m, slack)
        if broken:
            A[m - 1, n - slack] = 0.5
    return A


def _vecs(rng, count, k):
    return [rng.standard_normal(k) for _ in range(count)]


# ---------------------------------------------------------------- the argument list of every entry, by name and in order
# A value is an int, a float, an array (a pointer), a list of arrays (an array of pointers) or None (null).
def dense(entry, m, n, count=1, slack=0, broken=None, seed=0):
    """The per-member, shared and column-split entries.  slack: the hint passed to a *_slack entry; broken: the member whose
    matrix lacks the structure (0 for the one matrix of a single or shared upload)."""
    rng = np.random.default_rng(seed)
    name = "lpipm_upload" + entry
    lock, shared = "lockstep" in entry, "shared" in entry
    a = dict(c="ctx")
    if lock:
        a["count"] = count
    if entry == "_nsplit":
        a.update(m=m, n_total=2 * n, n_local=n, A=_mat(rng, m, n), lda=n, b=rng.standard_normal(m), cc=rng.standard_normal(n), c0=0.5)
        return name, a
    a.update(m=m, n=n)
    if lock and not shared:
        a.update(A=[_mat(rng, m, n, slack, broken == i) for i in range(count)])
    else:
        a.update(A=_mat(rng, m, n, slack, broken == 0), lda=n)
    if lock:
        a.update(b=_vecs(rng, count, m), cc=_vecs(rng, count, n), c0=rng.standard_normal(count))
    else:
        a.update(b=rng.standard_normal(m), cc=rng.standard_normal(n), c0=0.5)
    if entry.endswith("_slack"):
        a["n_slack"] = slack
    return name, a


def parts(entry, n, m_ub, m_eq=0, count=1, seed=0):
    """The ub / eq and the tall entries (tall: no `eq` arguments at all)."""
    rng = np.random.default_rng(seed)
    tall, shared = entry.endswith("_ub_tall"), "shared" in entry
    a = dict(c="ctx")
    if shared:
        a["count"] = count
    a.update(n=n, m_ub=m_ub, A_ub=_mat(rng, m_ub, n) if m_ub else None, lda_ub=n)
    if not shared:
        a["b_ub"] = rng.standard_normal(m_ub) if m_ub else None
    if not tall:
        a.update(m_eq=m_eq, A_eq=_mat(rng, m_eq, n) if m_eq else None, lda_eq=n)
        if not shared:
            a["b_eq"] = rng.standard_normal(m_eq) if m_eq else None
    if shared:
        a.update(b=_vecs(rng, count, m_ub + (0 if tall else m_eq)), cc=_vecs(rng, count, n), c0=rng.standard_normal(count))
    else:
        a.update(cc=rng.standard_normal(n), c0=0.5)
    return "lpipm_upload" + entry, a


def call(L, h, request, **override):
    """Calls the entry with its arguments, `override` replacing some by name.  -> return code"""
    name, args = request
    args = dict(args, **override)
    keep, argv = [], []
    for k, v in args.items():
        if k == "c":
            argv.append(h if v == "ctx" else None)
        elif isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v, dtype=np.float64)
            keep.append(v)
            argv.append(v.ctypes.data_as(_dp))
        elif isinstance(v, list):
            v = [np.ascontiguousarray(x, dtype=np.float64) for x in v]
            keep.append(v)
            argv.append((_dp * len(v))(*[x.ctypes.data_as(_dp) for x in v]))
        else:
            argv.append(v)
    for k, v in override.items():          # a null entry inside an otherwise valid pointer array
        if isinstance(v, NullAt):
            i = list(args).index(k)
            src = request[1][k]
            arr = (_dp * len(src))(*[x.ctypes.data_as(_dp) for x in src])
            arr[v.index] = _dp()
            keep.append(src)
            argv[i] = arr
    return int(getattr(L, name)(*argv))


# ---------------------------------------------------------------- the cases
ENTRIES_DENSE = ["", "_slack", "_lockstep", "_lockstep_slack", "_lockstep_shared", "_lockstep_shared_slack", "_nsplit"]
ENTRIES_PARTS = ["_ub_eq", "_lockstep_shared_ub_eq"]
ENTRIES_TALL = ["_ub_tall", "_lockstep_shared_ub_tall"]
CONFIGS = [(cache, scaling) for cache in (1, 0) for scaling in (0, 4)]


def size_requests():
    """(label, request): every entry over shapes that straddle one and two 128-row blocks."""
    out = []
    for m, n in ((96, 200), (130, 300)):
        for e in ENTRIES_DENSE:
            counts = (1, 3) if "lockstep" in e else (1,)
            for k in counts:
                if e.endswith("_slack"):
                    out.append((f"{e or '_'}:{m}x{n}:k{k}:hint", dense(e, m, n, k, slack=m)))
                    out.append((f"{e or '_'}:{m}x{n}:k{k}:hint_broken", dense(e, m, n, k, slack=m, broken=k - 1 if "shared" not in e else 0)))
                else:
                    out.append((f"{e or '_'}:{m}x{n}:k{k}", dense(e, m, n, k)))
    for m_ub, m_eq in ((60, 30), (60, 0), (0, 30)):
        for e in ENTRIES_PARTS:
            for k in ((1, 3) if "lockstep" in e else (1,)):
                out.append((f"{e}:n40:{m_ub}+{m_eq}:k{k}", parts(e, 40, m_ub, m_eq, k)))
    for n, m_ub in ((20, 300), (130, 1000)):
        for e in ENTRIES_TALL:
            for k in ((1, 3) if "lockstep" in e else (1,)):
                out.append((f"{e}:n{n}:{m_ub}:k{k}", parts(e, n, m_ub, 0, k)))
    return out


def sequences():
    """(label, [step, ...]); a step is ("cache", on), ("scaling", passes) or ("upload", request)."""
    up = lambda r: ("upload", r)
    return [
        ("same_padded_single", [up(dense("", 96, 200)), up(dense("", 90, 197))]),
        ("same_padded_slack", [up(dense("_slack", 96, 200, slack=96)), up(dense("_slack", 90, 194, slack=90))]),
        ("same_padded_lockstep", [up(dense("_lockstep", 96, 200, 3)), up(dense("_lockstep", 90, 197, 3))]),
        ("same_padded_shared", [up(dense("_lockstep_shared", 130, 300, 3)), up(dense("_lockstep_shared", 129, 290, 3))]),
        ("same_padded_ub_eq", [up(parts("_ub_eq", 40, 60, 30)), up(parts("_ub_eq", 39, 59, 28))]),
        ("same_padded_tall", [up(parts("_ub_tall", 20, 300)), up(parts("_ub_tall", 18, 290))]),
        ("same_padded_tall_other_mk", [up(parts("_ub_tall", 20, 300)), up(parts("_ub_tall", 32, 288))]),
        ("same_padded_shared_tall", [up(parts("_lockstep_shared_ub_tall", 20, 300, 0, 3)),
                                     up(parts("_lockstep_shared_ub_tall", 18, 290, 0, 3))]),
        ("cache_off_single", [up(dense("", 130, 300)), ("cache", 0), up(dense("", 130, 300)), ("cache", 1), up(dense("", 130, 300))]),
        ("cache_off_shared", [up(dense("_lockstep_shared", 96, 200, 3)), ("cache", 0), up(dense("_lockstep_shared", 96, 200, 3)),
                              ("cache", 1), up(dense("_lockstep_shared", 96, 200, 3))]),
        ("scaling_off_single", [("scaling", 4), up(dense("", 96, 200)), ("scaling", 0), up(dense("", 96, 200))]),
        ("scaling_off_lockstep", [("scaling", 4), up(dense("_lockstep", 96, 200, 3)), ("scaling", 0), up(dense("_lockstep", 96, 200, 3))]),
        ("scaling_off_shared", [("scaling", 4), up(dense("_lockstep_shared", 96, 200, 3)), ("scaling", 0),
                                up(dense("_lockstep_shared", 96, 200, 3))]),
        ("dense_tall_dense", [up(dense("", 130, 300)), up(parts("_ub_tall", 20, 300)), up(dense("", 130, 300))]),
        ("member_shared_member", [up(dense("_lockstep", 96, 200, 3)), up(dense("_lockstep_shared", 96, 200, 3)),
                                  up(dense("_lockstep", 96, 200, 3))]),
        ("shared_tall_shared", [up(dense("_lockstep_shared", 96, 200, 3)), up(parts("_lockstep_shared_ub_tall", 20, 300, 0, 3)),
                                up(dense("_lockstep_shared", 96, 200, 3))]),
        ("single_hint_nohint", [up(dense("_slack", 96, 200, slack=96)), up(dense("_slack", 96, 200, slack=96, broken=0)),
                                up(dense("", 96, 200))]),
    ]


def error_requests():
    """(label, request, override): every documented error of every entry, and the pairs that show precedence.  All of them
    are also made with a null context (host_cases)."""
    out = []
    base = [(e, dense(e, 4, 6, 3, slack=4 if e.endswith("_slack") else 0)) for e in ENTRIES_DENSE]
    base += [(e, parts(e, 3, 4, 2, 3)) for e in ENTRIES_PARTS] + [(e, parts(e, 2, 5, 0, 3)) for e in ENTRIES_TALL]
    for e, req in base:
        a = req[1]
        add = lambda what, **ov: out.append((f"{e or '_'}:{what}", req, ov))
        add("valid")
        for k, v in a.items():
            if isinstance(v, (np.ndarray, list)) or (k == "c0" and not isinstance(v, float)):
                add(f"null_{k}", **{k: None})
            if isinstance(v, list):
                add(f"null_{k}[1]", **{k: NullAt(1)})
        if "count" in a:
            add("count0", count=0)
            add("count4097", count=4097)
        for k in ("lda", "lda_ub", "lda_eq"):
            if k in a:
                add(f"{k}_short", **{k: a["n_local" if e == "_nsplit" else "n"] - 1})
        if "m" in a:
            add("m0", m=0)
            if "count" in a:
                add("count0_m0", count=0, m=0)
                add("count4097_m0", count=4097, m=0)
        if "m_ub" in a:
            zero = dict(m_ub=0) if "m_eq" not in a else dict(m_ub=0, m_eq=0)
            add("m0", **zero)
            add("m0_null_matrix", A_ub=None, **({"A_eq": None} if "m_eq" in a else {}), **zero)
            add("m_ub0_null_A_ub", m_ub=0, A_ub=None)
            add("null_A_ub_null_cc", A_ub=None, cc=None)
            if "m_eq" in a:
                add("m_eq0_null_A_eq", m_eq=0, A_eq=None)
                if "b_ub" in a:
                    add("m_ub0_null_b_ub", m_ub=0, A_ub=None, b_ub=None)
            if "count" in a:
                add("count0_m0", count=0, **zero)
                add("count4097_m0", count=4097, **zero)
                add("m0_null_b", b=None, **zero)
        if e == "_nsplit":
            add("n_local0", n_local=0)
            add("n_local_gt_total", n_local=a["n_total"] + 1)
            add("m0_n_local0", m=0, n_local=0)
        elif "n" in a:
            add("n0", n=0)
            add("m0_n0", **({"m": 0} if "m" in a else zero), n=0)
        if "n_slack" in a:
            add("n_slack_gt_n", n_slack=a["n"] + 1)
            add("n_slack_gt_m", n_slack=a["m"] + 1)
            add("m0_n_slack_gt_n", m=0, n_slack=a["n"] + 1)
    return out


def host_cases(L):
    """Every error request with a null context: nothing touches a device.  -> {label: return code}"""
    return {label: call(L, None, req, c=None, **ov) for label, req, ov in error_requests()}


_ALLREDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p)
_never_called = _ALLREDUCE(lambda *a: 1)


def device_cases(L):
    """-> {label: [return code, resident bytes]} ({label: [[rc, bytes], ...]} for a sequence), in a fixed order on contexts of
    their own.  An upload that is refused leaves what was resident: its bytes are part of the record."""
    def create():
        h = C.c_void_p()
        assert L.lpipm_create(0, C.byref(h)) == 0
        return h

    def bytes_of(h):
        out = C.c_uint64(0)
        assert L.lpipm_get_resident_bytes(h, C.byref(out)) == 0
        return int(out.value)

    rec = {}
    for cache, scaling in CONFIGS:
        h = create()
        assert L.lpipm_set_first_factor_cache(h, cache) == 0 and L.lpipm_set_scaling(h, scaling) == 0
        for label, req in size_requests():
            rc = call(L, h, req)
            rec[f"size:cache{cache}:scale{scaling}:{label}"] = [rc, bytes_of(h)]
        L.lpipm_destroy(h)
    for label, steps in sequences():
        h = create()
        got = []
        for kind, arg in steps:
            if kind == "cache":
                assert L.lpipm_set_first_factor_cache(h, arg) == 0
            elif kind == "scaling":
                assert L.lpipm_set_scaling(h, arg) == 0
            else:
                rc = call(L, h, arg)
                got.append([rc, bytes_of(h)])
        rec[f"seq:{label}"] = got
        L.lpipm_destroy(h)
    h = create()
    for label, req, ov in error_requests():
        rc = call(L, h, req, **ov)
        rec[f"err:{label}"] = [rc, bytes_of(h)]
    # a context of a column split (world 2) refuses the tall form, whatever else is wrong with the call
    assert L.lpipm_set_collective(h, 0, 2, C.cast(_never_called, C.c_void_p), None) == 0
    for e in ENTRIES_TALL:
        req = parts(e, 2, 5, 0, 3)
        for what, ov in (("valid", {}), ("m0", dict(m_ub=0)), ("null_A_ub", dict(A_ub=None)), ("null_cc", dict(cc=None))):
            rec[f"world2:{e}:{what}"] = [call(L, h, req, **ov), bytes_of(h)]
    assert L.lpipm_set_collective(h, 0, 1, None, None) == 0
    assert L.lpipm_set_scaling(h, 4) == 0
    rec["nsplit:scaling_on"] = [call(L, h, dense("_nsplit", 4, 6)), bytes_of(h)]
    L.lpipm_destroy(h)
    return rec


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def main():
    from lp_amd import _capi
    L = _capi.lib()
    doc = dict(note="recorded by tests/golden/make_upload_contract.py; device: label -> [return code, resident bytes]",
               cu_count=cu_count(), host=host_cases(L), device=device_cases(L))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(doc["host"]), "host cases,", len(doc["device"]), "device cases, CU count", doc["cu_count"])


if __name__ == "__main__":
    main()
