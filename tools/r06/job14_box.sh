#!/bin/bash
# box variance of the bench line: the full bench (no CPU baseline, no example legs) on a fresh box, one line per box in <output folder>
# usage: job14_box.sh <output folder>
O=${1:?usage: job14_box.sh <output folder>}; mkdir -p "$O"
python bench.py --full --no-cpu-baseline --no-extra-legs > "$O"/r06_box_$(date +%H%M).json 2>/dev/null
O="$O" python - <<'PY'
import json,glob,os
for f in sorted(glob.glob(os.path.join(os.environ['O'], 'r06_box_*.json'))):
    d=json.load(open(f)); t=d['target_262144']
    print(f, round(d['ms_per_step'],2), round(d['plain_ms_per_step'],2), round(d['roofline']['frac'],4), round(t['solve_wall_ms']['eliminate'],1), round(t['roofline']['elimination_frac'],4), round(d['batch_c4']['systems_per_s'],1))
PY
