#!/bin/bash
out=${OUT_DIR:-bench_out}
mkdir -p $out
( time timeout -k 10 900 python -m pytest tests/ -x -q -m gpu ) > $out/gputest_final.txt 2>&1
tail -n 6 $out/gputest_final.txt
python __graft_entry__.py smoke 2>&1 | tail -n 2      # build() then smoke() in one interpreter
python bench.py --full > $out/bench_final.json 2> $out/bench_final.err
python -c "
import json; d=json.load(open('$out/bench_final.json')); print(d['value'], d['ms_per_step'], d['step_hbm_frac']); print(d['roofline']); print(d['cpu_baseline']['value'], d['cpu_baseline']['cores'])"
