#!/bin/bash
# final state of round 6 on the DEFAULT build: rocprof captures (gen / enc / misc; serial-launch PMC passes + the benched schedule's
# kernel trace), every GPU test, the bench line, the encoder bench, the gates of the round's kernels
#   bash tools/r06_final.sh <results dir>   (the directory tools/capture_profiles.sh writes into)
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/r06_final.sh <results dir>}
bash tools/capture_profiles.sh prof_gen gen > $OUT/prof_gen.log 2>&1
bash tools/capture_profiles.sh prof_enc enc > $OUT/prof_enc.log 2>&1
bash tools/capture_misc.sh prof_misc > $OUT/prof_misc.log 2>&1
cd $GRAFT_REPO_ROOT
find $OUT/prof_gen $OUT/prof_enc $OUT/prof_misc -type f ! -name "*kernel_trace.csv" ! -name "*counter_collection.csv" ! -name "*kernel_stats.csv" -delete
mkdir -p $OUT/verify
(timeout 1800 python -m pytest tests -m gpu -q -rs 2>&1 | tail -25) > $OUT/verify/pytest.log 2>&1
(timeout 900 python bench.py --full 2> $OUT/verify/bench.err | tail -1) > $OUT/verify/bench.json
(for i in 1 2; do python tools/encode_bench.py --iters 40 2>/dev/null; done) > $OUT/verify/encode.txt
(timeout 600 python tools/lin128_gate.py 0 1 2>&1 | grep -v amdgpu.ids) > $OUT/verify/lin128_gate.txt
(timeout 600 python tools/conv2s128_gate.py 0 1 3 2>&1 | grep -v amdgpu.ids) > $OUT/verify/conv2s128_gate.txt
(BATCHES=1,2,4,8,16,32,64 python tools/batch_scaling.py 2>&1 | grep -v amdgpu.ids) > $OUT/verify/batch_scaling.txt
tail -4 $OUT/verify/pytest.log; head -c 300 $OUT/verify/bench.json; echo; cat $OUT/verify/encode.txt; tail -7 $OUT/verify/lin128_gate.txt; tail -6 $OUT/verify/conv2s128_gate.txt; cat $OUT/verify/batch_scaling.txt
