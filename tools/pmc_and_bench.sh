# The two rocprofv3 PMC passes of the level-0 kernels, their summary (profiles/pmc_latest.json, stamped with the library's source
# hash) and the bench line that reads it, in ONE run on one box: roofline.traffic_is_from_this_build is then true.
# usage: sh tools/pmc_and_bench.sh OUTDIR   (from anywhere; OUTDIR relative to the repository root)
# Every step must exit 0 or the script ends there: nothing more is started on a card after a fault, an abort or a time limit.
OUT=${1:?usage: tools/pmc_and_bench.sh OUTDIR}
cd "$(dirname "$0")/.." && mkdir -p "$OUT" && export TMPDIR=${TMPDIR:-/tmp} || exit 1
step() {
  "$@"
  rc=$?
  if [ $rc -ne 0 ]; then echo "stopping: exit status $rc from: $*" >&2; exit $rc; fi
}
export MG_FUSED=2
step timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_f" -o f -- python3 tools/kernel_probe.py 4097 10 jacobi sweeps2 down_leg up_leg span_leg span_leg_nomid > "$OUT/pmc_f.log" 2>&1
step timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_w" -o w -- python3 tools/kernel_probe.py 4097 10 jacobi sweeps2 down_leg up_leg span_leg span_leg_nomid > "$OUT/pmc_w.log" 2>&1
unset MG_FUSED
step python3 tools/pmc_summary.py "$OUT/pmc_f/f_counter_collection.csv" "$OUT/pmc_w/w_counter_collection.csv" profiles/pmc_latest.json > "$OUT/pmc_summary.log"
grep span "$OUT/pmc_summary.log"
step timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"
cp profiles/pmc_latest.json "$OUT/pmc_latest.json"
python -c "
import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);r=d['roofline'];print(d['value'],d['ms_per_step'],r['frac'],r['traffic'],r['traffic_is_from_this_build'],r['launch_ms'])" "$OUT/bench.json"
