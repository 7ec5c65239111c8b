#!/bin/bash
# usage: tools/gpu_pmc.sh "<counters pass 1>" ["<counters pass 2>" ...] — one rocprofv3 --pmc pass per argument on a short bench
# (every leg: --full); databases and logs go to $PMC_OUT (default: profile_out/pmc in the repository)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PMC_OUT=${PMC_OUT:-$ROOT/profile_out/pmc}
mkdir -p $PMC_OUT
cd /tmp && export TMPDIR=/tmp
i=0
for ctrs in "$@"; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --pmc $ctrs --kernel-trace -d $PMC_OUT/pmc_$i -o p -- python3 $ROOT/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $PMC_OUT/pmc_$i.log 2>&1
  echo "pass $i rc=$?"
done
ls -la $PMC_OUT/pmc_*/
