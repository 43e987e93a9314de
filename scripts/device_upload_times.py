#!/usr/bin/env python
"""Measurements behind profiles/device_upload.md (lpipm_upload_device).

Upload time, host entry against descriptor, 32 members that own their matrices:
  tall   lpipm_upload_lockstep_ub_tall against UB_TALL at 32 x 8192 x 128 and 32 x 4096 x 512; device sources contiguous,
         column-major and float32
  slack  lpipm_upload_lockstep against SLACK at 32 x 1024 x 2048; device source contiguous
One warm-up round, then five alternating rounds in one process; host clock around whole calls, each of which ends in a device
synchronise (the host arrays are pageable numpy arrays, the device sources torch tensors).
k_pack_matrix alone (lpipm_k_pack_matrix: HIP events around 20 back-to-back launches, beside hipMemcpyDtoDAsync of as many
bytes, timed the same way in the same process) at 32 x 8192 x 128 for the four copy modes: two elements per lane, one element
per lane (an odd element offset), LDS-transposed (column-major) and gather (a [::2, ::3] view).
  device_upload_times.py [tall:8192x128] [tall:4096x512] [slack:1024x2048] [pack:8192x128]     One JSON line on stdout."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lp_amd                      # noqa: E402

COUNT, ROUNDS, LAUNCHES = 32, 5, 20


def clock(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def sources(m, n):
    """[COUNT, m, n] normals on the device, and vectors of ones: an upload copies, it does not look at the values."""
    g = torch.Generator(device="cuda").manual_seed(1000 * m + n)
    A = torch.randn((COUNT, m, n), dtype=torch.float64, device="cuda", generator=g)
    ones = lambda k: torch.ones((COUNT, k), dtype=torch.float64, device="cuda")
    return A, ones(m), ones(n)


def layouts(A):
    col = A.transpose(1, 2).contiguous().transpose(1, 2)
    assert col.shape == A.shape and col.stride(1) == 1
    return {"contiguous": A, "column_major": col, "float32": A.float()}


def uploads(form, m, n):
    A, b, c = sources(m, n)
    nb = m
    hA, hb, hc = list(A.cpu().numpy()), list(b.cpu().numpy()), list(c.cpu().numpy())
    host, dev = lp_amd.Context(0), lp_amd.Context(0)
    if form == "tall":
        ways = {"host": lambda: host.upload_lockstep_ub_tall(hA, hb, hc)}
        for name, v in layouts(A).items():
            bb, cc = (b.float(), c.float()) if v.dtype == torch.float32 else (b, c)
            ways["device_" + name] = (lambda v=v, bb=bb, cc=cc: dev.upload_device(v, bb, cc, form="ub_tall"))
    else:
        ways = {"host": lambda: host.upload_lockstep(hA, hb, hc),
                "device_contiguous": lambda: dev.upload_device(A, b, c)}
    for f in ways.values():                                            # warm-up: code objects loaded, allocations made
        f()
    rounds = [{k: clock(f) for k, f in ways.items()} for _ in range(ROUNDS)]
    out = {"members": COUNT, "m": m, "n": n, "len_b": nb, "matrix_bytes_f64": COUNT * m * n * 8,
           "resident_bytes": {"host": host.resident_bytes(), "device": dev.resident_bytes()}, "rounds_s": rounds,
           "median_s": {k: float(np.median([r[k] for r in rounds])) for k in ways},
           "device_contiguous_faster_in_every_round": all(r["device_contiguous"] < r["host"] for r in rounds)}
    out["host_over_device_contiguous"] = out["median_s"]["host"] / out["median_s"]["device_contiguous"]
    host.close(); dev.close()
    return out


def pack(m, n):
    A, b, c = sources(m, n)
    cx = lp_amd.Context(0)
    odd = torch.empty(COUNT * m * n + 1, dtype=torch.float64, device="cuda")[1:].view(COUNT, m, n)
    odd.copy_(A)
    big = torch.zeros((COUNT, 2 * m, 3 * n), dtype=torch.float64, device="cuda")
    gather = big[:, ::2, ::3]
    gather.copy_(A)
    views = {"row_two_per_lane": A, "row_one_per_lane": odd, "lds_transposed": layouts(A)["column_major"], "gather": gather,
             "row_two_per_lane_float32": A.float()}
    out = {"members": COUNT, "m": m, "n": n, "launches": LAUNCHES, "modes": {}}
    for name, v in views.items():
        bb, cc = (b.float(), c.float()) if v.dtype == torch.float32 else (b, c)
        cx.upload_device(v, bb, cc, form="ub_tall")
        cx.k_pack_matrix(v, bb, cc, repeats=LAUNCHES, form="ub_tall")                  # warm-up
        pack_ms, copy_ms = cx.k_pack_matrix(v, bb, cc, repeats=LAUNCHES, form="ub_tall")
        moved = COUNT * m * n * (v.element_size() + 8)                                # bytes read plus bytes written
        out["modes"][name] = {"pack_ms": pack_ms, "copy_ms": copy_ms, "bytes_read_plus_written": moved,
                              "pack_GBps": moved / pack_ms / 1e6, "copy_GBps": moved / copy_ms / 1e6,
                              "pack_over_copy_time": pack_ms / copy_ms}
    cx.close()
    return out


if __name__ == "__main__":
    todo = sys.argv[1:] or ["tall:8192x128", "tall:4096x512", "slack:1024x2048", "pack:8192x128"]
    res = {}
    for item in todo:
        kind, shape = item.split(":")
        m, n = (int(v) for v in shape.split("x"))
        res[item] = pack(m, n) if kind == "pack" else uploads(kind, m, n)
    print(json.dumps(res))
