#!/bin/bash
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}; mkdir -p "$OUT"; export OUT     # where the lines and logs go
timeout 900 python -m pytest tests/test_gpu_parity2.py -x -q -m gpu -k "carried_old" 2>&1 | tail -4
timeout 900 python -m pytest tests/test_gpu_parity.py -x -q -m gpu 2>&1 | tail -4
timeout 600 python bench.py --full --steps 5 --warmup 2 --cpu-sample 0 --no-e2e > "$OUT"/c25_bench.json 2> "$OUT"/c25_bench.err; echo rc=$?
python - <<'PY'
import json, os
j = json.loads(open(os.path.join(os.environ["OUT"], "c25_bench.json")).read().strip().splitlines()[-1])
print(j["ms_per_step"], j["config"]["harmony_iterations"], j["roofline"]["avg_block_step_us"])
print(j["config"]["gpu_phase_ms_per_step"])
PY
HMX_SOLD_CARRY=0 timeout 600 python bench.py --full --steps 5 --warmup 2 --cpu-sample 0 --no-e2e > "$OUT"/c25_bench0.json 2> "$OUT"/c25_bench0.err; echo rc=$?
python - <<'PY'
import json, os
j = json.loads(open(os.path.join(os.environ["OUT"], "c25_bench0.json")).read().strip().splitlines()[-1])
print("carry off:", j["ms_per_step"], j["config"]["harmony_iterations"], j["roofline"]["avg_block_step_us"])
print(j["config"]["gpu_phase_ms_per_step"])
PY
