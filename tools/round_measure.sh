#!/bin/bash
# End-of-round measurement on one GPU: rocprof passes (humanoid, aloha_cloth), then the bench line of
# every config into $OUT/bench_<model>.log.  Stops at the first failing step.
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
bash tools/gpu_profile.sh || exit $?
bash tools/gpu_profile_sparse.sh aloha_cloth || exit $?
timeout -k 10 300 python -u bench.py --full > $OUT/bench_humanoid.log 2>&1 || exit $?
for mdl in franka apollo cloth; do
  timeout -k 10 300 python -u bench.py --full --model $mdl --cpu-baseline 0 > $OUT/bench_$mdl.log 2>&1 || exit $?
done
timeout -k 10 300 python -u bench.py --full --model aloha_cloth > $OUT/bench_aloha_cloth.log 2>&1 || exit $?
for mdl in humanoid franka apollo cloth aloha_cloth; do
  python3 -c "import json;d=json.loads(open('$OUT/bench_$mdl.log').read().splitlines()[-1]);r=d['roofline'];print('$mdl', round(d['value'],1), 'ms/step', round(d['ms_per_step'],4), 'kernel_ms', round(r['kernel_ms'],4), 'frac', round(r['frac'],4), 'traffic', r['traffic'], 'cpu', (d['cpu_baseline'] or {}).get('value'))"
done
