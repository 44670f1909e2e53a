#!/bin/bash
# Round 6, first lease: the RCCL init A/B, the whole GPU suite in the driver's own form, the full bench line.
# usage: job01_suite_rccl_bench.sh <output folder>
O=${1:?usage: job01_suite_rccl_bench.sh <output folder>}; mkdir -p "$O"
python tools/r06/rccl_init_ab.py "lease $(date +%H%M)" >> "$O"/r06_rccl_init.txt 2>&1
( time python -m pytest tests/ -x -q -m gpu --durations=15 ) > "$O"/r06a_pytest.log 2>&1
tail -30 "$O"/r06a_pytest.log
python bench.py --full > "$O"/r06a_bench.json 2> "$O"/r06a_bench.err
tail -c 600 "$O"/r06a_bench.json
cat "$O"/r06_rccl_init.txt
