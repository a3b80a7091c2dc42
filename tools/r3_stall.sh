#!/bin/bash
# results under $OUT (default runs/)
set -eo pipefail
export OUT=${OUT:-runs}
mkdir -p $OUT
for r in 1 2 3 4 5 6; do python bench.py --full --steps 10 --warmup 3 --cpu-outfits 0 > $OUT/stall_$r.json 2>/dev/null; done
python - <<'PY'
import json, glob, os
for f in sorted(glob.glob(os.path.join(os.environ['OUT'], 'stall_*.json'))):
    d = json.loads([l for l in open(f) if l.startswith('{')][-1]); s = d['step_ms_spread']
    print(f.split('/')[-1], d['ms_per_step'], 'allocs', s['device_allocs_in_timed_region'], s['all'], 'host', s['host_issue_ms'])
PY
