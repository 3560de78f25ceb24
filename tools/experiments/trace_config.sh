#!/usr/bin/env bash
# Kernel trace of one single-pair config's registrations (run on the GPU box):
#   tools/experiments/trace_config.sh <C1|C2|C5> [name]    -> $OUT_DIR/tc_<name>/  (default _var/out)
set -eu
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
export TMPDIR=/tmp
CFG=$1; NAME=${2:-$1}
OUT_DIR=${OUT_DIR:-_var/out}
mkdir -p "$OUT_DIR"
timeout -k 10 240 rocprofv3 --kernel-trace -d "$OUT_DIR/tc_$NAME" -o run --output-format csv -- \
    python3 bench.py --full --plan-from-env --no-c3 --no-cpu --check 0 --configs "$CFG" > "$OUT_DIR/tc_$NAME.log" 2>&1
echo "trace_config: $NAME done"
