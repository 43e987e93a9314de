#!/bin/bash
# Two built trees of this repository side by side on one GPU, alternating: bench.py (C3 it/s), bench.py --workload c2 (the
# 512x1024 LP, it/s: the solve most sensitive to host overhead), bench.py --workload c4 (LP/s) and upload_times.py, ROUNDS times
# each per tree.  usage: compare_trees.sh <tree A> <tree B> [ROUNDS=5] > log
# Every GPU step runs under its own time limit and the first failure ends the run.  One result line per step:
#   <tree label> <step> <the step's JSON line>
set -o pipefail
a=$(cd "$1" && pwd) || exit 2; b=$(cd "$2" && pwd) || exit 2; rounds=${3:-5}
step() {   # tree label, step name, tree, seconds, command...
    local label=$1 name=$2 tree=$3 limit=$4 line; shift 4
    line=$(cd "$tree" && timeout -k 10 "$limit" "$@" 2>/dev/null | grep '^{' | tail -1) || { echo "FAILED: $label $name (status $?)"; exit 1; }
    echo "$label $name $line"
}
for r in $(seq "$rounds"); do
    for t in A B; do
        tree=$a; [ $t = B ] && tree=$b
        step $t c3 "$tree" 300 python bench.py --gpus 1 --steps 5 --warmup 1
        step $t c2 "$tree" 300 python bench.py --gpus 1 --steps 5 --warmup 1 --workload c2
        step $t c4 "$tree" 300 python bench.py --gpus 1 --steps 5 --warmup 1 --workload c4
        step $t upload "$tree" 300 python scripts/upload_times.py
    done
done
