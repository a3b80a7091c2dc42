#!/bin/bash
# A/B of two builds of the library on the headline bench, alternating processes on one box:  bash tools/lib_ab.sh outfitx_amd/libofx_hip_exp.so
# lines and results under $OUT (default runs/)
set -eo pipefail
export OUT=${OUT:-runs}
EXP=$(pwd)/$1; mkdir -p $OUT
for r in 1 2; do
  python bench.py --full --steps 10 --warmup 3 --cpu-outfits 0 > $OUT/ab_base_$r.json 2>/dev/null
  OFX_LIB=$EXP python bench.py --full --steps 10 --warmup 3 --cpu-outfits 0 > $OUT/ab_exp_$r.json 2>/dev/null
done
python - <<'PY'
import json, glob, os
for f in sorted(glob.glob(os.path.join(os.environ['OUT'], 'ab_*.json'))):
    d = json.loads([l for l in open(f) if l.startswith('{')][-1])
    sh = {(r['M'], r['N'], r['K']): r['us_per_launch'] for r in d['roofline']['per_shape'] if r['kernel'] == 'gemm_w2f8_kernel'}
    print(f.split('/')[-1], d['ms_per_step'], d['step_ms_spread']['median'], ' '.join(f"{k[1]}x{k[2]}:{v}" for k, v in sh.items()))
PY
