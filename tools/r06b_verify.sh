#!/bin/bash
# last verification of the round: every GPU test, the bench line (with the committed PMC capture of this build), the encoder bench
#   bash tools/r06b_verify.sh <results dir>
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/r06b_verify.sh <results dir>}
mkdir -p $OUT/verify
(timeout 1800 python -m pytest tests -m gpu -q -rs 2>&1 | tail -25) > $OUT/verify/pytest.log 2>&1
(timeout 900 python bench.py --full 2> $OUT/verify/bench.err | tail -1) > $OUT/verify/bench.json
(for i in 1 2; do python tools/encode_bench.py --iters 40 2>/dev/null; done) > $OUT/verify/encode.txt
python -c "import __graft_entry__ as g; g.smoke()" > $OUT/verify/smoke.txt 2>&1; echo "smoke rc=$?" >> $OUT/verify/smoke.txt
tail -3 $OUT/verify/pytest.log; head -c 400 $OUT/verify/bench.json; echo; cat $OUT/verify/encode.txt; tail -2 $OUT/verify/smoke.txt
