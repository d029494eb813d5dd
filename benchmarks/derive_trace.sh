#!/bin/bash
# One kernel trace of the ingest's gather and the derive gathers (benchmarks/derive_trace.py) -> the table on stdout.
#   bash benchmarks/derive_trace.sh [output directory]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-/tmp/derive_trace}
rm -rf "$OUT"
mkdir -p "$OUT"
timeout -k 10 400 rocprofv3 --kernel-trace --output-format csv -d "$OUT/t" -- python "$ROOT/benchmarks/derive_trace.py" > "$OUT/run.log" 2>&1
python "$ROOT/benchmarks/derive_trace.py" --summarize "$OUT/t"
