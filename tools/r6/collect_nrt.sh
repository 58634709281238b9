#!/bin/bash
set -u
cd /root/repo
for batch in "config3 config3_most config3_balanced" "config3_leastnuma config3_r8 config3_r8_balanced" "config5_share config2_lroc"; do
  rm -rf gpurun_out/prof_*
  /usr/local/graft/bin/gpurun --timeout 1500 -- "bash tools/prof_all.sh $batch 2>&1 | tail -4" 2>&1 | grep -E "status=" | tail -2
  python tools/collect_profiles.py r06 $batch 2>&1 | tail -4
done
rm -rf gpurun_out/prof_*
OUT=${OUT:-bench_out}/r6
mkdir -p "$OUT"
timeout 1800 python bench.py --workload config5 --gpus 1 --steps 3 --warmup 1 --sweep-only --cpu-budget 0 --full > "$OUT/config5_full_bench_line.json" 2> "$OUT/config5_full.err"
python -c "import json, sys; d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('config5 whole', d['roofline']['kernel_ms'], d.get('every_row', {}).get('kernel_ms'))" "$OUT/config5_full_bench_line.json"
cp "$OUT/config5_full_bench_line.json" profiles/r06/
