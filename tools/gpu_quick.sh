#!/bin/bash
# quick check on an MI355X: parity tests (output kept in $OUT/quick_tests.log) + one bench line
OUT=${OUT:-results}; mkdir -p $OUT
python -m pytest ${QUICK_TESTS:-tests/test_gpu_parity.py tests/test_gpu_lm.py} -m gpu -x -q > $OUT/quick_tests.log 2>&1; tail -3 $OUT/quick_tests.log
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline "$@" > $OUT/b3.log 2>&1; python - <<EOP
import json
d=json.loads([l for l in open("$OUT/b3.log") if l.startswith("{")][-1])
print(d["value"], {k:round(v["avg_ms"],4) for k,v in d["kernels"].items()}, d["residual_rel"])
EOP
