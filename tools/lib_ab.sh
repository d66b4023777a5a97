#!/bin/bash
# A/B of two builds of the library on one box, alternating DISSC_HIP_LIB (B = dissc_amd/libdissc_hip_alt.so)
#   tools/lib_ab.sh [rounds] [leg]
#     leg = headline (default): generator forward, bench.py's headline loop -> ms_per_step, audio-sec/sec
#     leg = latency: bench.py's B = 1 latency leg (a dependent chain of launches: host bound) -> median ms at T = 100, T = 500
# Stops at the first run that fails or exceeds its time limit.
set -eo pipefail
R=${1:-3}
LEG=${2:-headline}
case $LEG in
  headline) ARGS="--no-latency"; PICK="j['ms_per_step'], j['value']" ;;
  latency) ARGS="--full"; PICK="j['latency']['T100']['ms'], j['latency']['T500']['ms']" ;;
  *) echo "lib_ab.sh: leg must be headline or latency" >&2; exit 2 ;;
esac
for r in $(seq 1 $R); do
  for lib in "" dissc_amd/libdissc_hip_alt.so; do
    DISSC_HIP_LIB=$lib timeout -k 10 300 python bench.py --steps 30 --warmup 5 --no-cpu-baseline --no-pipeline --no-strong --no-split-bf16 --no-d2h $ARGS 2>/dev/null \
      | python -c "import sys,json; j=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('${lib:-default}', $PICK)"
  done
done
