#!/usr/bin/env bash
# Development aid (GPU box): the resident pipeline's step under library variants, alternating, LAB_ROUNDS rounds (default 3).
#   scripts/lab_step.sh <tag> <lib>[+VAR=VALUE] [<lib>[+VAR=VALUE] ...]        (lib: product | lab/libgfm_X.so)
# +VAR=VALUE: an environment variable for that arm alone (e.g. lab/libgfm_X.so+GRAFIMO_SCORE_OVERLAP=0).
# LAB_BENCH_ARGS: arguments of bench.py (default: the lean resident-pipeline run).  Every run has its own time limit and
# the first one that fails ends the script.
set -o pipefail
root="$GRAFT_REPO_ROOT"; tag="$1"; shift; out="$root/gpurun_out/$tag.txt"; cd "$root"
mkdir -p "$(dirname "$out")"; : > "$out"
for round in $(seq 1 "${LAB_ROUNDS:-3}"); do
  for arm in "$@"; do
    lib="${arm%%+*}"; setenv=(); [ "$arm" != "$lib" ] && setenv=("${arm#*+}")
    unset GRAFIMO_HIP_LIB; [ "$lib" != "product" ] && export GRAFIMO_HIP_LIB="$root/$lib"
    env "${setenv[@]}" timeout -k 10 "${LAB_STEP_LIMIT:-120}" python3 bench.py ${LAB_BENCH_ARGS:---no-cpu-baseline --no-e2e --no-extras} 2>/dev/null | tail -1 | python3 -c "
import json,sys
d=json.loads(sys.stdin.read()); r=d['roofline']; t=d.get('tail_ms') or {}
print('%-26s value %.4g  step %.2f us  kernel %.2f us  gap %.2f us  tail avg %.1f max %.1f us' % ('$arm', d['value'], 1e3*d['ms_per_step'], 1e3*r['kernel_ms_avg'], 1e3*(d['ms_per_step']-r['kernel_ms_avg']), 1e3*t.get('avg',0), 1e3*t.get('max',0)))" | tee -a "$out" || { echo "$arm: run failed, stopping" | tee -a "$out"; exit 1; }
  done
done
