#!/bin/bash
# GPU job: the new host-arena tests + the end-to-end update figure with its host timeline
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${1:-$(mktemp -d)}; mkdir -p "$OUT"          # (the logs and the bench line go to the folder named by the first argument)
python -m pytest tests/test_host_rlft.py -x -q -m gpu 2>&1 | tail -5 > "$OUT/e2e_tests.log"
python bench.py --steps 20 --full --no-cpu-baseline --no-precisions --no-roofline > "$OUT/e2e_bench.json" 2> "$OUT/e2e_bench.err"
tail -3 "$OUT/e2e_tests.log"; python -c "
import json, sys; d=json.load(open(sys.argv[1])); print(json.dumps(d.get('full_update_e2e'), indent=1)); print(d['ms_per_step'], d.get('full_update'))" "$OUT/e2e_bench.json"
tail -5 "$OUT/e2e_bench.err"
