#!/bin/bash
# A/B of prebuilt libraries (tools/ab_build.sh -> tools/_ab/lib_<tag>.so) on the four workloads of the bench line:
#   tools/ab_run.sh <reps> tag1 tag2 ...   prints trajectories/s (thousands): default run | the driver's call | configs[2] | configs[4]
# Every bench.py run has a time limit (AB_TIMEOUT seconds, default 600); the first run that fails ends the A/B with the
# tail of its stderr.
reps=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root" || exit 1
limit=${AB_TIMEOUT:-600}
err=$(mktemp)
trap 'rm -f "$err"' EXIT
run() {  # run <label> <bench.py arguments ...>
  local label=$1; shift
  local out rc
  out=$(timeout -k 10 "$limit" python bench.py "$@" 2> "$err")
  rc=$?
  if [ $rc -ne 0 ]; then
    echo; echo "$label: bench.py $* exited with status $rc"; tail -n 20 "$err"
    exit $rc
  fi
  echo -n "$label $(printf '%s\n' "$out" | tail -n 1 | python3 -c "import sys, json; print(round(json.loads(sys.stdin.read())['value'] / 1e3, 1))") "
}
for rep in $(seq 1 "$reps"); do for t in "$@"; do
  lib=$root/tools/_ab/lib_$t.so
  [ -f "$lib" ] || { echo "no $lib (tools/ab_build.sh $t)"; exit 1; }
  export GTO_HIP_LIB=$lib
  echo -n "$t: "
  run "default" --no-cpu-baseline --no-other-configs --no-next-rows --merged-launches-only
  run "| steps20" --steps 20 --warmup 5 --no-cpu-baseline --no-other-configs --no-next-rows --merged-launches-only
  run "| cfg2" --light --no-cpu-baseline --no-next-rows --no-other-configs --repeats 3 --warmup 1 --robot fetch --batch 256 --shelf --merge 8 --steps 32
  run "| cfg4" --light --no-cpu-baseline --no-next-rows --no-other-configs --repeats 3 --warmup 1 --robot fetch_mobile --T 80 --grid 256 --shelf --batch 64 --merge 8 --steps 32
  echo; done; done
