"""Records the solve contract: what every solve entry of the C ABI returns and leaves in its outputs.

solve_contract.json : per case the return code of the call and per member [status, iterations, sha256 of fun's bytes, sha256 of
                      x's bytes]; where a member has no x, "untouched" if its sentinel-filled row is still all sentinel.  A null
                      output array is recorded as "null".  Each distinct member record is stored once (pack / load below).  Plus the CU count of the device it was recorded on (kernel plans, and
                      with them the bits of a solve, depend on it).
                      tests/test_gpu_solve_contract.py replays the `device` cases on the code under test and
                      tests/test_solve_contract_host.py the `host` ones (a null context: no device is touched); both require
                      equality.

The record is the behaviour of the commit it was taken at: regenerate it only at a commit whose results and return codes are
the intended ones (before a change that must keep them), never to make a failing replay pass.  Only public entries are
called, so the script runs unchanged at any commit that has them.
Run from the repo root on an MI355X:  python tests/golden/make_solve_contract.py
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "solve_contract.json")

_dp, _u64p, _i32p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
SENT, SENT_ITS, SENT_ST = -7.25, 12345, -99     # what every output holds before the call
INF, UNB = "infeasible", "unbounded"
FAKE_DEV = 4096                                 # a non-null "device pointer" of the calls that must never reach a device


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _p(a):
    return a.ctypes.data_as(_dp)


def _parr(vs):
    """An array of pointers to the given arrays; a None entry is a null pointer."""
    arr = (_dp * max(len(vs), 1))()
    for i, v in enumerate(vs):
        if v is not None:
            arr[i] = _p(v)
    return arr


# ---------------------------------------------------------------- members
def dense_member(m, n, seed, kind=None):
    """The project's planted LP in slack form (A m x n); INF: row 0 >= 0 with b[0] = -1; UNB: a free column of cost -1."""
    from lp_amd import synth
    A, b, c, _ = synth.planted_lp(seed, m, n)
    if kind == INF:
        A[0, :] = np.abs(A[0, :]); b[0] = -1.0
    if kind == UNB:
        A[:, 0] = 0.0; c[0] = -1.0
    return A, b, c


def ub_member(m, nx, seed, kind=None):
    """X (m x nx), b, c of a pure-`ub` LP as tests/test_gpu_tall_batches.py plants it: row 0 >= 0 and column 0 <= 0, so b[0] = -1
    makes it infeasible and c[0] = -1 unbounded."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((m, nx))
    X[0, :] = np.abs(X[0, :]); X[:, 0] = -np.abs(X[:, 0]); X[0, 0] = 0.0
    k = min(nx // 2, m)
    xs = np.zeros(nx); xs[:k] = rng.uniform(1, 2, k)
    act = rng.permutation(m)[:k]
    s = rng.uniform(1, 2, m); s[act] = 0.0
    b = X @ xs + s
    lam = np.zeros(m); lam[act] = rng.uniform(1, 2, k)
    mu = np.zeros(nx); mu[k:] = rng.uniform(1, 2, nx - k)
    c = -X.T @ lam + mu
    if kind == INF:
        b[0] = -1.0
    if kind == UNB:
        c[0] = -1.0
    return X, b, c


def hinted_member(m, n, seed, kind=None, broken=False):
    """[X I] of m x n with n_slack = m; broken: one entry of the slack block is not the identity's."""
    X, b, c = ub_member(m, n - m, seed, kind)
    A = np.hstack([X, np.eye(m)])
    if broken:
        A[m - 1, n - m] = 0.5
    return np.ascontiguousarray(A), b, np.concatenate([c, np.zeros(m)])


def kinds(count):
    """From count 3 on member 1 is infeasible and the last one unbounded."""
    return [INF if (count >= 3 and i == 1) else UNB if (count >= 3 and i == count - 1) else None for i in range(count)]


def dense_list(m, n, count, seed0=0):
    return [dense_member(m, n, seed0 + i, k) for i, k in enumerate(kinds(count))]


# ---------------------------------------------------------------- calls
def opts_of(L, **kw):
    from lp_amd import _capi
    o = _capi.Opts()
    L.lpipm_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


class XBlock:
    """Sentinel-filled destinations of `count` solutions: host rows (null_rows: those members' pointers are null), or one
    block on the device (`stride` doubles per row), or a fake device pointer that nothing may touch."""
    def __init__(self, lens, where, stride=None, null_rows=()):
        self.lens, self.where, self.null_rows = list(lens), where, set(null_rows)
        self.stride = stride if stride is not None else max(self.lens + [1])
        self.rows = self.block = None
        if where == "host":
            self.rows = [np.full(k, SENT) for k in self.lens]
        elif where == "device":
            import torch
            self.block = torch.full((max(len(self.lens), 1), max(self.stride, max(self.lens + [1]))), SENT, dtype=torch.float64, device="cuda")

    def host_arg(self):
        if self.where != "host":
            return None
        return _parr([None if i in self.null_rows else r for i, r in enumerate(self.rows)])

    def dev_arg(self):
        if self.where == "device":
            return C.c_void_p(self.block.data_ptr())
        return C.c_void_p(FAKE_DEV) if self.where == "fake" else None

    def digest(self, i, k, has_x):
        """What member i's destination holds: the hash of its k doubles when the member has a solution."""
        if self.where == "host":
            row = self.rows[i]
        elif self.where == "device":
            import torch
            torch.cuda.synchronize()
            flat = self.block.reshape(-1).cpu().numpy()
            row = flat[i * self.stride: i * self.stride + k]
        else:
            return "none"
        if has_x and i not in self.null_rows:
            return _sha(row)
        return "untouched" if np.all(row == SENT) else "touched:" + _sha(row)


class Outs:
    """fun / iterations / status arrays of `count` members, sentinel-filled; `null`: the names of those passed as null."""
    def __init__(self, count, null=()):
        k = max(count, 1)
        self.count, self.null = count, set(null)
        self.fun, self.its, self.st = np.full(k, SENT), np.full(k, SENT_ITS, dtype=np.uint64), np.full(k, SENT_ST, dtype=np.int32)

    def args(self):
        return (None if "fun" in self.null else _p(self.fun),
                None if "its" in self.null else self.its.ctypes.data_as(_u64p),
                None if "st" in self.null else self.st.ctypes.data_as(_i32p))

    def members(self, xb, lens):
        out = []
        for i in range(self.count):
            st = int(self.st[i])
            out.append([st, "null" if "its" in self.null else int(self.its[i]),
                        "null" if "fun" in self.null else _sha(self.fun[i:i + 1]), xb.digest(i, lens[i], st in (0, 7))])
        return out


def solve_single(L, h, n, where, log=False, **okw):
    """lpipm_solve (where = "host") / lpipm_solve_device ("device", or "null": no destination) on what is resident."""
    from lp_amd import _capi
    o = opts_of(L, **okw)
    xb = XBlock([n], "device" if where == "device" else "host")
    fun, its = np.full(1, SENT), np.full(1, SENT_ITS, dtype=np.uint64)
    rows = (_capi.IterRow * int(min(o.max_iter, 1000)))() if log else None
    if where == "host":
        rc = L.lpipm_solve(h, C.byref(o), _p(xb.rows[0]), _p(fun), its.ctypes.data_as(_u64p), rows)
    else:
        rc = L.lpipm_solve_device(h, C.byref(o), xb.dev_arg() if where == "device" else None, _p(fun), its.ctypes.data_as(_u64p), rows)
    rec = dict(rc=int(rc), members=[[int(rc), int(its[0]), _sha(fun), xb.digest(0, n, rc in (0, 7))]])
    if log:
        rec["log"] = hashlib.sha256(bytes(rows)).hexdigest()
    return rec


def solve_lockstep(L, h, count, n, where, stride=None, null_rows=(), null=(), **okw):
    o = opts_of(L, **okw)
    lens = [n] * count
    xb, out = XBlock(lens, where, stride, null_rows), Outs(count, null)
    if where in ("host", "hostnull"):         # hostnull: the host entry without its array of rows
        rc = L.lpipm_solve_lockstep(h, C.byref(o), xb.host_arg(), *out.args())
    else:
        rc = L.lpipm_solve_lockstep_device(h, C.byref(o), xb.dev_arg(), xb.stride, *out.args())
    return dict(rc=int(rc), members=out.members(xb, lens))


def upload_lockstep(L, h, members, c0=None):
    m, n = members[0][0].shape
    keep = [np.ascontiguousarray(v) for mem in members for v in mem]
    rc = L.lpipm_upload_lockstep(h, len(members), m, n, _parr(keep[0::3]), _parr(keep[1::3]), _parr(keep[2::3]), None if c0 is None else _p(c0))
    assert rc == 0, rc
    return n


def solve_batch(L, h, entry, members, where, hints=None, stride=None, c0=None, null=(), null_in=(), count=None, both=False, **okw):
    """entry: "" | "_device" | "_slack" | "_ub_tall".  members: [(A, b, c)], A m x n (tall: the m_ub x n block, x has n + m_ub
    entries).  null_in: names among m n A b c (and n_slack) passed as null.  both: host rows AND a device block."""
    tall = entry == "_ub_tall"
    o = opts_of(L, **okw)
    k = len(members)
    count = k if count is None else count
    ms = np.array([mem[0].shape[0] for mem in members] + [0], dtype=np.uint64)
    ns = np.array([mem[0].shape[1] for mem in members] + [0], dtype=np.uint64)
    lens = [int(ns[i] + (ms[i] if tall else 0)) for i in range(k)]
    keep = [[np.ascontiguousarray(mem[j], dtype=np.float64) for mem in members] for j in range(3)]
    arg = dict(m=ms.ctypes.data_as(_u64p), n=ns.ctypes.data_as(_u64p), A=_parr(keep[0]), b=_parr(keep[1]), c=_parr(keep[2]))
    hint_arr = np.array(list(hints if hints is not None else [0] * k) + [0], dtype=np.uint64)
    arg["n_slack"] = hint_arr.ctypes.data_as(_u64p) if hints is not None else None
    for name in null_in:
        arg[name] = None
    stride = max(lens + [1]) if stride is None else stride
    xh = XBlock(lens, "host") if (where == "host" or both) else None
    xd = XBlock(lens, where, stride) if where in ("device", "fake") else (XBlock(lens, "fake", stride) if both else None)
    out = Outs(k, null)
    c0p = None if c0 is None else _p(c0)
    head = [h, count, arg["m"], arg["n"]] + ([arg["n_slack"]] if entry == "_slack" else []) + [arg["A"], arg["b"], arg["c"], c0p, C.byref(o)]
    if entry == "":
        rc = L.lpipm_solve_batch(*head, xh.host_arg() if xh else None, *out.args())
    elif entry == "_device":
        rc = L.lpipm_solve_batch_device(*head, xd.dev_arg() if xd else None, stride, *out.args())
    else:
        rc = getattr(L, "lpipm_solve_batch" + entry)(*head, xh.host_arg() if xh else None, xd.dev_arg() if xd else None, stride, *out.args())
    xb = xd if (xd and where != "host") else xh if xh else XBlock(lens, "none")
    return dict(rc=int(rc), members=out.members(xb, lens))


# ---------------------------------------------------------------- the cases
def mixed_dense():
    """five 24x40 (one infeasible, one unbounded), two 40x72 and one lone shape, interleaved"""
    a, b, lone = dense_list(24, 40, 5), dense_list(40, 72, 2, 50), dense_member(30, 50, 70)
    return [a[0], b[0], a[1], a[2], lone, a[3], b[1], a[4]]


def mixed_tall():
    a = [ub_member(64, 8, 200 + i, k) for i, k in enumerate(kinds(3))]
    b = [ub_member(300, 40, 210 + i) for i in range(2)]
    return [a[0], b[0], a[1], ub_member(50, 6, 220), b[1], a[2]]


def hinted_list():
    return [hinted_member(96, 200, 300 + i, k) for i, k in enumerate(kinds(3))]


def argument_errors(L, h, where_dev):
    """Every argument error of the batch and lockstep entries, on context h (null: nothing reaches a device; where_dev is
    then "fake").  -> {label: record}"""
    rec = {}
    dense, tall, hinted = dense_list(24, 40, 2), [ub_member(64, 8, 200 + i) for i in range(2)], hinted_list()[:1] * 2
    per = {"": dense, "_device": dense, "_slack": hinted, "_ub_tall": tall}
    for e, mem in per.items():
        where = where_dev if e == "_device" else "host"
        hints = [96, 96] if e == "_slack" else None
        base = dict(hints=hints)
        rec[f"batch{e}:valid"] = solve_batch(L, h, e, mem, where, **base)
        rec[f"batch{e}:count0"] = solve_batch(L, h, e, mem, where, count=0, **base)
        rec[f"batch{e}:null_status"] = solve_batch(L, h, e, mem, where, null=("st",), **base)
        rec[f"batch{e}:null_fun_its"] = solve_batch(L, h, e, mem, where, null=("fun", "its"), **base)
        for name in ("m", "n", "A", "b", "c"):
            rec[f"batch{e}:null_{name}"] = solve_batch(L, h, e, mem, where, null_in=(name,), **base)
        if e != "":
            short = mem[0][0].shape[1] - 1 + (mem[0][0].shape[0] if e == "_ub_tall" else 0)
            rec[f"batch{e}:stride_short"] = solve_batch(L, h, e, mem, where_dev, stride=short, **base)
            rec[f"batch{e}:stride_short_null_n"] = solve_batch(L, h, e, mem, where_dev, stride=short, null_in=("n",), **base)
            rec[f"batch{e}:stride_short_null_status"] = solve_batch(L, h, e, mem, where_dev, stride=short, null=("st",), **base)
        if e in ("", "_device"):
            rec[f"batch{e}:no_x"] = solve_batch(L, h, e, mem, "none", **base)
            rec[f"batch{e}:no_x_count0"] = solve_batch(L, h, e, mem, "none", count=0, **base)
        else:
            rec[f"batch{e}:both_x"] = solve_batch(L, h, e, mem, "host", both=True, **base)
            rec[f"batch{e}:neither_x"] = solve_batch(L, h, e, mem, "none", **base)
            rec[f"batch{e}:neither_x_count0"] = solve_batch(L, h, e, mem, "none", count=0, **base)
            rec[f"batch{e}:both_x_null_status"] = solve_batch(L, h, e, mem, "host", both=True, null=("st",), **base)
            rec[f"batch{e}:device_block"] = solve_batch(L, h, e, mem, where_dev, **base)
    return rec


def host_cases(L):
    """Every argument error with a null context, and the single and lockstep entries on one.  -> {label: record}"""
    rec = {f"null_ctx:{k}": v for k, v in argument_errors(L, None, "fake").items()}
    rec["null_ctx:solve"] = solve_single(L, None, 40, "host")
    rec["null_ctx:solve_device_null_x"] = solve_single(L, None, 40, "null")
    rec["null_ctx:lockstep_host"] = solve_lockstep(L, None, 3, 40, "host")
    rec["null_ctx:lockstep_device"] = solve_lockstep(L, None, 3, 40, "fake")
    rec["null_ctx:lockstep_device_null_x"] = solve_lockstep(L, None, 3, 40, "none")
    return rec


def device_cases(L):
    """-> {label: record}, in a fixed order on contexts of their own."""
    def create():
        h = C.c_void_p()
        assert L.lpipm_create(0, C.byref(h)) == 0
        return h

    rec = {}
    # ---- single solves
    h = create()
    rec["single:nothing_uploaded"] = solve_single(L, h, 40, "host")
    A, b, c = dense_member(24, 40, 0)
    X, bt, ct = ub_member(64, 8, 200)
    Ah, bh, ch = hinted_member(96, 200, 300)
    rng = np.random.default_rng(5)
    Aub, Aeq = rng.standard_normal((24, 16)), rng.standard_normal((6, 16))
    xs = rng.uniform(0, 1, 16)
    bub, beq, cue = Aub @ xs + rng.uniform(0.5, 1, 24), Aeq @ xs, rng.uniform(1, 2, 16)
    uploads = {
        "dense": (40, lambda: L.lpipm_upload(h, 24, 40, _p(A), 40, _p(b), _p(c), 0.5)),
        "dense40x72": (72, lambda: (lambda m: L.lpipm_upload(h, 40, 72, _p(m[0]), 72, _p(m[1]), _p(m[2]), 0.0))(dense_member(40, 72, 50))),
        "infeasible": (40, lambda: (lambda m: L.lpipm_upload(h, 24, 40, _p(m[0]), 40, _p(m[1]), _p(m[2]), 0.5))(dense_member(24, 40, 1, INF))),
        "unbounded": (40, lambda: (lambda m: L.lpipm_upload(h, 24, 40, _p(m[0]), 40, _p(m[1]), _p(m[2]), 0.5))(dense_member(24, 40, 4, UNB))),
        "hinted": (200, lambda: L.lpipm_upload_slack(h, 96, 200, _p(Ah), 200, _p(bh), _p(ch), 0.25, 96)),
        "ub_eq": (40, lambda: L.lpipm_upload_ub_eq(h, 16, 24, _p(Aub), 16, _p(bub), 6, _p(Aeq), 16, _p(beq), _p(cue), 0.0)),
        "tall": (72, lambda: L.lpipm_upload_ub_tall(h, 8, 64, _p(X), 8, _p(bt), _p(ct), 1.5)),
        "tall300x40": (340, lambda: (lambda m: L.lpipm_upload_ub_tall(h, 40, 300, _p(m[0]), 40, _p(m[1]), _p(m[2]), 0.0))(ub_member(300, 40, 210))),
    }
    for name, (n, up) in uploads.items():
        assert up() == 0, name
        for where in ("host", "device", "null"):
            for log in (False, True):
                rec[f"single:{name}:{where}:log{int(log)}"] = solve_single(L, h, n, where, log)
    assert uploads["dense"][1]() == 0
    for kw in (dict(max_iter=1), dict(max_iter=3), dict(ip=0), dict(solver_type=1), dict(solver_type=2), dict(solver_type=3),
               dict(solver_type=-1), dict(alpha0=0.0), dict(alpha0=1.0), dict(tol=0.0), dict(alpha0=1.0, solver_type=3)):
        label = ",".join(f"{k}={v}" for k, v in kw.items())
        rec[f"single:dense:{label}"] = solve_single(L, h, 40, "host", True, **kw)
        rec[f"single:dense:{label}:device"] = solve_single(L, h, 40, "device", False, **kw)
    assert uploads["tall"][1]() == 0
    for kw in (dict(max_iter=2), dict(ip=0), dict(solver_type=1), dict(solver_type=2)):
        label = ",".join(f"{k}={v}" for k, v in kw.items())
        rec[f"single:tall:{label}"] = solve_single(L, h, 72, "host", True, **kw)
    assert L.lpipm_set_scaling(h, 4) == 0 and uploads["hinted"][1]() == 0
    rec["single:hinted:scaling4"] = solve_single(L, h, 200, "host", True)
    rec["single:hinted:scaling4:device"] = solve_single(L, h, 200, "device")
    assert L.lpipm_set_scaling(h, 0) == 0
    upload_lockstep(L, h, dense_list(24, 40, 3))
    rec["single:on_lockstep_batch"] = solve_single(L, h, 40, "host")
    rec["single:on_lockstep_batch:qr"] = solve_single(L, h, 40, "host", solver_type=1)
    L.lpipm_destroy(h)
    h = create()                                   # a column split of world 1
    assert L.lpipm_set_collective(h, 0, 1, None, None) == 0
    assert L.lpipm_upload_nsplit(h, 24, 40, 40, _p(A), 40, _p(b), _p(c), 0.5) == 0
    for where in ("host", "device"):
        for log in (False, True):
            rec[f"single:nsplit:{where}:log{int(log)}"] = solve_single(L, h, 40, where, log)
    rec["single:nsplit:max_iter=2"] = solve_single(L, h, 40, "host", True, max_iter=2)
    rec["lockstep:on_nsplit"] = solve_lockstep(L, h, 1, 40, "host")
    L.lpipm_destroy(h)

    # ---- lockstep solves
    h = create()
    rec["lockstep:nothing_uploaded"] = solve_lockstep(L, h, 3, 40, "host")
    for count in (1, 3, 15, 16, 17):
        n = upload_lockstep(L, h, dense_list(24, 40, count), np.arange(count, dtype=np.float64))
        rec[f"lockstep:k{count}:host"] = solve_lockstep(L, h, count, n, "host")
        rec[f"lockstep:k{count}:host_again"] = solve_lockstep(L, h, count, n, "host")           # replays the kept first factor
        rec[f"lockstep:k{count}:host_null_row"] = solve_lockstep(L, h, count, n, "host", null_rows=(0,))
        rec[f"lockstep:k{count}:device"] = solve_lockstep(L, h, count, n, "device", stride=n)
        rec[f"lockstep:k{count}:device_wide"] = solve_lockstep(L, h, count, n, "device", stride=n + 5)
        rec[f"lockstep:k{count}:device_short"] = solve_lockstep(L, h, count, n, "device", stride=n - 1)
        rec[f"lockstep:k{count}:qr"] = solve_lockstep(L, h, count, n, "host", solver_type=1)
        rec[f"lockstep:k{count}:max_iter3"] = solve_lockstep(L, h, count, n, "device", stride=n, max_iter=3)
        rec[f"lockstep:k{count}:null_fun_its"] = solve_lockstep(L, h, count, n, "host", null=("fun", "its"))
        rec[f"lockstep:k{count}:null_status"] = solve_lockstep(L, h, count, n, "host", null=("st",))
        rec[f"lockstep:k{count}:no_x"] = solve_lockstep(L, h, count, n, "none")
        rec[f"lockstep:k{count}:no_rows"] = solve_lockstep(L, h, count, n, "hostnull")
        rec[f"lockstep:k{count}:no_x_short"] = solve_lockstep(L, h, count, n, "none", stride=n - 1)
        rec[f"lockstep:k{count}:bad_tol"] = solve_lockstep(L, h, count, n, "host", tol=0.0)
    for count in (3, 17):
        assert L.lpipm_set_first_factor_cache(h, 0) == 0
        n = upload_lockstep(L, h, dense_list(24, 40, count))
        rec[f"lockstep:k{count}:cache_off"] = solve_lockstep(L, h, count, n, "host")
        rec[f"lockstep:k{count}:cache_off_again"] = solve_lockstep(L, h, count, n, "host")
        assert L.lpipm_set_first_factor_cache(h, 1) == 0 and L.lpipm_set_scaling(h, 4) == 0
        n = upload_lockstep(L, h, dense_list(24, 40, count))
        rec[f"lockstep:k{count}:scaling4"] = solve_lockstep(L, h, count, n, "host")
        rec[f"lockstep:k{count}:scaling4:device"] = solve_lockstep(L, h, count, n, "device", stride=n + 5)
        assert L.lpipm_set_scaling(h, 0) == 0
    tall = [ub_member(64, 8, 200 + i, k) for i, k in enumerate(kinds(17))]
    keep = [np.ascontiguousarray(v) for mem in tall for v in mem]
    assert L.lpipm_upload_lockstep_ub_tall(h, 17, 8, 64, _parr(keep[0::3]), 8, _parr(keep[1::3]), _parr(keep[2::3]), None) == 0
    rec["lockstep:tall_own:k17:host"] = solve_lockstep(L, h, 17, 72, "host")
    rec["lockstep:tall_own:k17:device_short"] = solve_lockstep(L, h, 17, 72, "device", stride=71)
    assert L.lpipm_upload(h, 24, 40, _p(A), 40, _p(b), _p(c), 0.5) == 0
    rec["lockstep:on_single_upload"] = solve_lockstep(L, h, 1, 40, "host")
    L.lpipm_destroy(h)

    # ---- batch solves
    mixed, mtall, hinted = mixed_dense(), mixed_tall(), hinted_list()
    c0 = np.arange(8, dtype=np.float64) / 4
    h = create()
    for lock in (-1, 0, 2, 3):
        assert L.lpipm_set_batch_lockstep(h, lock) == 0
        for conc in ((0, 1, 3) if lock in (-1, 2) else (0,)):
            assert L.lpipm_set_batch_concurrency(h, conc) == 0
            tag = f"lock{lock}:conc{conc}"
            rec[f"batch:mixed:{tag}:host"] = solve_batch(L, h, "", mixed, "host", c0=c0)
            rec[f"batch:mixed:{tag}:device"] = solve_batch(L, h, "_device", mixed, "device", c0=c0, stride=77)
            rec[f"batch:tall:{tag}:host"] = solve_batch(L, h, "_ub_tall", mtall, "host", c0=c0)
        assert L.lpipm_set_batch_concurrency(h, 0) == 0
        rec[f"batch:mixed:lock{lock}:slack_entry_host"] = solve_batch(L, h, "_slack", mixed, "host", hints=None)
        rec[f"batch:mixed:lock{lock}:slack_entry_device"] = solve_batch(L, h, "_slack", mixed, "device", hints=[0] * 8, c0=c0)
        rec[f"batch:tall:lock{lock}:device"] = solve_batch(L, h, "_ub_tall", mtall, "device", stride=345)
        # hints: three that hold (one infeasible, one unbounded member), one that does not hold, one larger than n, one dense
        hm = hinted + [hinted_member(96, 200, 310, broken=True), hinted_member(96, 200, 311), dense_member(24, 40, 0)]
        rec[f"batch:hints:lock{lock}:host"] = solve_batch(L, h, "_slack", hm, "host", hints=[96, 96, 96, 96, 201, 0], c0=c0)
        rec[f"batch:hints:lock{lock}:device"] = solve_batch(L, h, "_slack", hm, "device", hints=[96, 96, 96, 96, 97, 41])
        rec[f"batch:mixed:lock{lock}:qr"] = solve_batch(L, h, "", mixed, "host", solver_type=1)
        rec[f"batch:mixed:lock{lock}:max_iter3"] = solve_batch(L, h, "_device", mixed, "device", max_iter=3)
        rec[f"batch:mixed:lock{lock}:bad_alpha0"] = solve_batch(L, h, "", mixed, "host", alpha0=1.0)
        rec[f"batch:mixed:lock{lock}:null_fun_its"] = solve_batch(L, h, "", mixed, "host", null=("fun", "its"))
        # a tall member on a QR arm is UNSUPPORTED, a runtime code that stops the handing out: one worker, so that which members
        # were handed out before it does not depend on the threads' timing
        assert L.lpipm_set_batch_concurrency(h, 1) == 0
        rec[f"batch:tall:lock{lock}:qr"] = solve_batch(L, h, "_ub_tall", mtall, "host", solver_type=2)
        assert L.lpipm_set_batch_concurrency(h, 0) == 0
        # a member without rows (Unconstrained), alone and beside a group
        empty = (np.zeros((0, 40)), np.zeros(0), np.ones(40))
        rec[f"batch:m0:lock{lock}"] = solve_batch(L, h, "", [mixed[0], empty, mixed[2], empty], "host")
        rec[f"batch:m0:lock{lock}:tall"] = solve_batch(L, h, "_ub_tall", [mtall[0], (np.zeros((0, 8)), np.zeros(0), np.ones(8)), mtall[2]], "device")
        rec[f"batch:m0:lock{lock}:hint"] = solve_batch(L, h, "_slack", [hinted[0], empty, hinted[2]], "host", hints=[96, 5, 96])
    assert L.lpipm_set_batch_lockstep(h, -1) == 0
    for count in (17, 33):                      # the default group size: 9 + 8, and 32 with one member left over
        mem = dense_list(24, 40, count)
        rec[f"batch:equal{count}:host"] = solve_batch(L, h, "", mem, "host")
        rec[f"batch:equal{count}:device"] = solve_batch(L, h, "_device", mem, "device", c0=np.arange(count, dtype=np.float64))
        tl = [ub_member(64, 8, 200 + i, k) for i, k in enumerate(kinds(count))]
        rec[f"batch:equal{count}:tall"] = solve_batch(L, h, "_ub_tall", tl, "host")
    assert L.lpipm_set_scaling(h, 4) == 0
    rec["batch:mixed:scaling4"] = solve_batch(L, h, "_device", mixed, "device", c0=c0)
    rec["batch:tall:scaling4"] = solve_batch(L, h, "_ub_tall", mtall, "host")
    assert L.lpipm_set_scaling(h, 0) == 0
    rec.update({f"args:{k}": v for k, v in argument_errors(L, h, "device").items()})
    L.lpipm_destroy(h)
    return rec


def cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


# ---------------------------------------------------------------- the file
# The library is deterministic and a member's results do not depend on the call it is part of, so the same member record
# recurs in many cases.  The file holds every distinct record once (`records`) and a case as [rc, [record index per member]]
# (a logged single solve: [rc, [index], sha256 of the log]); load() gives the cases back as device_cases / host_cases make them.
def pack(doc):
    records, index = [], {}

    def case(r):
        ids = []
        for m in r["members"]:
            key = json.dumps(m)
            if key not in index:
                index[key] = len(records)
                records.append(m)
            ids.append(index[key])
        return [r["rc"], ids] + ([r["log"]] if "log" in r else [])
    out = dict(note=doc["note"], cu_count=doc["cu_count"])
    for part in ("host", "device"):
        out[part] = {k: case(doc[part][k]) for k in sorted(doc[part])}
    out["records"] = records
    return out


def unpack(packed):
    def case(c):
        r = dict(rc=c[0], members=[packed["records"][i] for i in c[1]])
        if len(c) > 2:
            r["log"] = c[2]
        return r
    return dict(note=packed["note"], cu_count=packed["cu_count"], host={k: case(c) for k, c in packed["host"].items()},
                device={k: case(c) for k, c in packed["device"].items()})


def save(doc, path=OUT):
    """One line per record and per case."""
    p = pack(doc)
    line = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:
        f.write('{"note":%s,\n"cu_count":%d,\n' % (json.dumps(p["note"]), p["cu_count"]))
        for part in ("host", "device"):
            f.write('"%s":{\n%s\n},\n' % (part, ",\n".join("%s:%s" % (json.dumps(k), line(c)) for k, c in p[part].items())))
        f.write('"records":[\n%s\n]}\n' % ",\n".join(line(m) for m in p["records"]))


def load(path=OUT):
    with open(path) as f:
        return unpack(json.load(f))


def main():
    from lp_amd import _capi
    L = _capi.lib()
    doc = dict(note="recorded by tests/golden/make_solve_contract.py; a record is [status, iterations, sha256(fun), "
                    "sha256(x) | untouched]",
               cu_count=cu_count(), host=host_cases(L), device=device_cases(L))
    save(doc)
    assert load() == doc
    seen = sorted({m[0] for r in doc["device"].values() for m in r["members"]})
    print(len(doc["host"]), "host cases,", len(doc["device"]), "device cases, CU count", doc["cu_count"], "statuses", seen)


if __name__ == "__main__":
    main()
