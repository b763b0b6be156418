#!/bin/bash
# On the GPU box: the three measurements of DESIGN.md 4.5 into one text file ($OUT, default ./huffopt.txt).
#   1. symbol_histogram_kernel beside code_tiles_kernel in ONE rocprofv3 --kernel-trace --stats run (4096x4096, noise and smooth)
#   2. code_tiles_kernel of every ab/libjpezy_<name>.so (tools/ab/ab_build.py; e.g. the parent commit's build next to this one),
#      setting off, interleaved over ROUNDS rounds
#   3. wall time and file size of jpezy_write_jpeg_gpu with the setting off and on
# Every step runs under its own time limit; the script stops at the first step that fails.
set -u
OUT=$(realpath -m "${OUT:-$PWD/huffopt.txt}")
mkdir -p "$(dirname "$OUT")"
: > $OUT
ROOT=$PWD
export TMPDIR=/tmp
stats() {   # $1: label, JPEZY_LIB from the environment
  rm -rf /tmp/rp_ho
  (cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_ho -o ho -- python3 $ROOT/tools/measure/measure_huffopt.py --trace > /dev/null 2>&1) || return 1
  f=$(find /tmp/rp_ho -name '*kernel_stats.csv' | head -1)
  python3 - "$f" "$1" <<'PY' | tee -a $OUT
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if any(k in r["Name"] for k in ("symbol_histogram", "code_tiles", "assemble", "stuff_kernel")):
        print(f"  {sys.argv[2]} {r['Name'][:70]:70s} calls={r['Calls']:>3s} avg_us={float(r['AverageNs'])/1e3:7.2f} min_us={float(r['MinNs'])/1e3:7.2f}")
PY
}
echo "== 1. kernels of one trace (this build)" | tee -a $OUT
stats this || { echo "trace failed" | tee -a $OUT; exit 1; }
if ls ab/libjpezy_*.so > /dev/null 2>&1; then
  echo "== 2. code_tiles_kernel, A/B interleaved" | tee -a $OUT
  for round in $(seq 1 ${ROUNDS:-3}); do
    for lib in $ROOT/ab/libjpezy_*.so; do
      name=$(basename $lib .so); name=${name#libjpezy_}
      JPEZY_LIB=$lib stats "round$round $name" || { echo "trace of $name failed" | tee -a $OUT; exit 1; }
    done
  done
fi
echo "== 3. cost and gain of the option" | tee -a $OUT
timeout -k 10 240 python3 tools/measure/measure_huffopt.py 2>&1 | tee -a $OUT
exit ${PIPESTATUS[0]}
