# The measurements of a round in one run on one box: GPU tests, the full bench line, its kernel trace, the PMC passes of the
# level-0 kernels, the W-cycle trace and the per-configuration times.
# usage: sh tools/run_round_measurements.sh OUTDIR   (from anywhere; OUTDIR relative to the repository root)
# Every step must exit 0 or the script ends there: nothing more is started on a card after a fault, an abort or a time limit.
# The GPU tests alone may also return 1 (tests failed, the process itself ended normally).
set -x
OUT=${1:?usage: tools/run_round_measurements.sh OUTDIR}
cd "$(dirname "$0")/.." && mkdir -p "$OUT" && export TMPDIR=${TMPDIR:-/tmp} || exit 1
step() {
  "$@"
  rc=$?
  if [ $rc -ne 0 ]; then echo "stopping: exit status $rc from: $*" >&2; exit $rc; fi
}
timeout -k 10 900 python -m pytest tests -m gpu -q > "$OUT/gpu_tests.log" 2>&1
rc=$?
tail -6 "$OUT/gpu_tests.log"
if [ $rc -gt 1 ]; then echo "stopping: GPU tests exit status $rc" >&2; exit $rc; fi
step timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
tail -c 600 "$OUT/bench.json"
step timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_bench" -o bench -- python3 bench.py --full --steps 20 --no-cpu-baseline > "$OUT/prof_bench.log" 2>&1
export MG_FUSED=2
step timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_f" -o f -- python3 tools/kernel_probe.py 4097 10 jacobi sweeps2 down_leg up_leg span_leg span_leg_nomid > "$OUT/pmc_f.log" 2>&1
step timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_w" -o w -- python3 tools/kernel_probe.py 4097 10 jacobi sweeps2 down_leg up_leg span_leg span_leg_nomid > "$OUT/pmc_w.log" 2>&1
unset MG_FUSED
step timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_w" -o w -- python3 tools/wcycle_probe.py > "$OUT/prof_w.log" 2>&1
step timeout -k 10 400 python tools/config_times.py all > "$OUT/config_times.log" 2>&1
cat "$OUT/config_times.log"
find "$OUT" -name "*.csv" | head -30
