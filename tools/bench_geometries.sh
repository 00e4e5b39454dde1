#!/bin/bash
# Run on an MI355X: bench lines + rocprofv3 kernel summaries for the reference geometry (16x4000, utility.h:50-55) and for config 5's
# geometry (64x2048 with a 200-key-frame local map).  Outputs $OUT/<round>_geo_* (default prof_out/); copy to profiles/ afterwards.
set -eu   # a failing step ends the script: no GPU run is started after it
R=${1:-r06}
ROOT=$(cd "$(dirname "$0")/.." && pwd)   # the repository this script belongs to
OUT=${OUT:-prof_out}                     # relative to the repository
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
mkdir -p "$OUT"
run() {  # tag, bench args...
  local tag=$1; shift
  timeout 1200 python bench.py "$@" --full --no-cpu < /dev/null > $OUT/${R}_geo_${tag}.json 2> $OUT/${R}_geo_${tag}.err
  rm -rf /tmp/prof_geo
  timeout 1200 rocprofv3 --kernel-trace --stats -d /tmp/prof_geo -o st --output-format csv -- python bench.py "$@" --full --no-cpu --no-profile < /dev/null > $OUT/${R}_geo_${tag}_under_rocprof.json 2> /tmp/geo.log
  find /tmp/prof_geo -name "*kernel_stats.csv" -exec cp {} $OUT/${R}_geo_${tag}_kernel_stats.csv \;
  # HBM traffic per launch: two separate --pmc passes (FETCH_SIZE, WRITE_SIZE), as tools/refresh_profiles.sh does for the default workload
  local per=$(python - <<PY
import json
d = json.loads(open("$OUT/${R}_geo_${tag}.json").read().strip().splitlines()[-1])
print(d["roofline"]["streams_per_launch"])
PY
)
  for c in FETCH_SIZE WRITE_SIZE; do
    rm -rf /tmp/pmcg_$c
    timeout 1200 rocprofv3 --pmc $c --kernel-trace -d /tmp/pmcg_$c -o p --output-format csv -- python bench.py "$@" --steps 8 --warmup 0 --no-cpu --no-profile --no-check --no-isolated < /dev/null > /tmp/pmcg_$c.log 2>&1
  done
  python tools/pmc_traffic.py /tmp/pmcg_FETCH_SIZE /tmp/pmcg_WRITE_SIZE "$per" 16 > $OUT/${R}_geo_${tag}_pmc_traffic.json
  tail -c 600 $OUT/${R}_geo_${tag}.json; echo; head -8 $OUT/${R}_geo_${tag}_kernel_stats.csv
}
run 16x4000 --geometry 16x4000 --kf-cap 16384 --streams 2304 --steps 60 --warmup 10
run 64x2048_k200 --geometry 64x2048 --keyframes 200 --kf-cap 8192 --streams 768 --bags 4 --prime 2400 --steps 40 --warmup 10
# SQ instruction counters of config 5's geometry, every kernel alone on the chip (ImageProjection's share of the VALU instructions)
bash tools/pmc_geo_sq.sh $OUT/${R}_geo_64x2048_pmc_sq.json
ls -la $OUT/${R}_geo_*
