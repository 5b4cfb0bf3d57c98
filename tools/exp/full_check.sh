#!/bin/bash
# full GPU validation of the current build: parity suite, fuzz, per-layer times, bench line (--full)
#   tools/exp/full_check.sh [output directory, default full_check_out]
set -o pipefail
O=${1:-full_check_out}
mkdir -p "$O"
timeout -k 10 900 python -m pytest tests -x -q -m gpu < /dev/null > "$O/fc_pytest.log" 2>&1 || { tail -30 "$O/fc_pytest.log"; exit 1; }
tail -2 "$O/fc_pytest.log"
if grep -q "Memory access fault" "$O/fc_pytest.log"; then exit 9; fi
timeout -k 10 300 python tests/fuzz/fuzz_parity.py 300 < /dev/null > "$O/fc_fuzz.log" 2>&1 || { tail -30 "$O/fc_fuzz.log"; exit 2; }
tail -2 "$O/fc_fuzz.log"
timeout -k 10 200 python tools/bench_layers.py < /dev/null > "$O/fc_layers.log" 2>&1 || { tail -30 "$O/fc_layers.log"; exit 3; }
grep -E "conv|deconv|pmap|sum|total" "$O/fc_layers.log" | tail -30
timeout -k 10 600 python bench.py --full < /dev/null > "$O/fc_bench.json" 2> "$O/fc_bench.err" || { tail -30 "$O/fc_bench.err"; exit 4; }
cat "$O/fc_bench.json"
if grep -q "Memory access fault" "$O"/fc_*.log "$O/fc_bench.err"; then exit 9; fi
