#!/bin/bash
# round-3 validation sequence on the GPU box: full GPU suite -> headline bench -> rocprofv3 passes -> the other BASELINE configs
# (results under $OUT, default runs/)
set -eo pipefail
export OUT=${OUT:-runs}
mkdir -p $OUT
python -m pytest tests -m gpu -x -q > $OUT/final_gpu_tests.log 2>&1 || { tail -30 $OUT/final_gpu_tests.log; exit 1; }
tail -2 $OUT/final_gpu_tests.log
python bench.py --full > $OUT/final_bench.json 2> $OUT/final_bench.err || { tail -20 $OUT/final_bench.err; exit 1; }
python - <<'PY'
import json, os
d = json.loads([l for l in open(os.path.join(os.environ['OUT'], 'final_bench.json')) if l.startswith('{')][-1])
print({k: d[k] for k in ('value', 'ms_per_step', 'step_ms_spread', 'parity_rel_err_vs_reference')}); print(d['roofline']['achieved'], d['roofline']['frac'], d['cpu_baseline'])
PY
bash tools/profile_r03.sh > $OUT/final_profile.log 2>&1 || { tail -20 $OUT/final_profile.log; exit 1; }
python tools/bench_configs.py > $OUT/final_configs.jsonl 2> $OUT/final_configs.err || { tail -20 $OUT/final_configs.err; exit 1; }
cat $OUT/final_configs.jsonl | cut -c1-300
