#!/bin/bash
# full GPU test suite, then the bench with every row (--full); logs under $OUT_DIR (default /tmp/commu_round)
cd "$(dirname "$0")/../.."
out=${OUT_DIR:-/tmp/commu_round}
mkdir -p "$out"
timeout 1500 python -m pytest tests -m gpu -x -q > "$out/gpu_tests.log" 2>&1; echo "tests rc=$?" >> "$out/gpu_tests.log"
tail -15 "$out/gpu_tests.log"
timeout 900 python bench.py --full "$@" > "$out/bench_full.json" 2> "$out/bench_full.err"; echo "bench rc=$?"
tail -5 "$out/bench_full.err"
BENCH_JSON="$out/bench_full.json" python - <<'PY'
import json, os
d = json.load(open(os.environ["BENCH_JSON"]))
print(json.dumps({k: d[k] for k in ("value", "ms_per_step", "roofline")}, indent=None))
for k, v in d.get("extra_rows", {}).items():
    print(k, v["value"], v["ms_per_step"], v["step_mfma_frac"], v["roofline"]["kernel"], v["roofline"]["frac"])
print(json.dumps(d.get("decode", {}))[:1500])
print(d.get("cpu_baseline"))
PY
