#!/bin/bash
# C4 / C5 sweep over the number of trunk streams of the frozen ViT
CFG=${1:-c4}
R=${GRAFT_REPO_ROOT:-$PWD}
for s in 2 3 4; do
  CVCL_VIT_TRUNK_STREAMS=$s python3 $R/bench.py --config $CFG --steps 40 --warmup 10 --no-cpu-baseline --no-parity --no-roofline --no-extras 2>/dev/null | python3 -c "
import json,sys; d=json.loads(sys.stdin.read()); print('streams $s', '$CFG', d['value'], d['ms_per_step'])"
done
