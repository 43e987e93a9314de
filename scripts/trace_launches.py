"""The launches of a rocprofv3 --kernel-trace run, reduced to what two trees can be compared by: per stream (of every process of
the run), in dispatch order, the kernel name with its grid and workgroup sizes; the streams' sequences sorted by length, then
text.  Prints the text, or with --hash one line: launches per stream, distinct kernels, SHA-1 of the text (12 hex digits).
The three templated kernels of kernels_tall.hip are written by the names their instantiations had as separate kernels.
usage: trace_launches.py [--hash] DIR   (every *kernel_trace.csv under DIR)"""
import csv
import glob
import hashlib
import os
import re
import sys

TALL = re.compile(r"k_tall_(setup|pq_uv|uv_corr)<(true|false)>")


def name_of(raw):
    raw = raw[5:] if raw.startswith("void ") else raw
    return TALL.sub(lambda m: ("k_tall_eq_" if m.group(2) == "true" else "k_tall_") + m.group(1), raw)


def sequences(directory):
    seqs = []
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)):
        rows = list(csv.DictReader(open(path)))
        order = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
        stream = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
        rows.sort(key=lambda r: int(r[order]))
        per = {}
        for r in rows:
            grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
            wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
            per.setdefault(r[stream], []).append(f"{name_of(r['Kernel_Name'])} grid {grid} wg {wg}")
        seqs += list(per.values())
    return sorted(seqs, key=lambda s: (len(s), "\n".join(s)))


if __name__ == "__main__":
    seqs = sequences(sys.argv[-1])
    text = "".join(f"--- stream of {len(s)} launches\n" + "\n".join(s) + "\n" for s in seqs)
    if "--hash" in sys.argv:
        kernels = {l.split(" grid ")[0] for s in seqs for l in s}
        print(" + ".join(str(len(s)) for s in seqs) or "0", len(kernels), hashlib.sha1(text.encode()).hexdigest()[:12])
    else:
        sys.stdout.write(text)
