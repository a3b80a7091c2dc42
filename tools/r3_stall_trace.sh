#!/bin/bash
# results under $OUT (default runs/)
set -eo pipefail
ROOT=$(pwd); export OUT=$ROOT/${OUT:-runs}; mkdir -p $OUT; rm -rf $OUT/st
python3 bench.py --full --cpu-outfits 0 > $OUT/st_plain.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --output-format csv -d $OUT/st -- python3 $ROOT/bench.py --full --cpu-outfits 0 > $OUT/st.log 2>&1
cd $ROOT
python3 tools/trace_stalls.py $(find $OUT/st -name "*kernel_trace.csv" | head -1) > $OUT/stall_trace.txt
rm -rf $OUT/st
python3 - <<'PY'
import json, os
for f in (os.path.join(os.environ['OUT'], 'st_plain.json'), os.path.join(os.environ['OUT'], 'st.log')):
    l = [x for x in open(f) if x.startswith('{"metric')][-1]; d = json.loads(l); s = d['step_ms_spread']
    print(f, d['ms_per_step'], 'median', s['median'], [x for x in s['all'] if x > 40])
PY
cat $OUT/stall_trace.txt
