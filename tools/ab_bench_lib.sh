#!/bin/bash
# A/B of a variant library on the full prover: parity tests with the variant,
# then alternating benches (variant, in-tree, variant, in-tree).
# Usage (GPU box): bash tools/ab_bench_lib.sh gpurun_ab/libqpgpu_X.so NAME
cd "$(dirname "$0")/.."; OUT=${QP_OUT_DIR:-bench_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
lib=$1; name=$2
QPGPU_LIB=$lib timeout -k 10 600 python -u -m pytest tests/test_gpu_prover.py tests/test_gpu_reference_proof.py tests/test_gpu_seams.py -x -q --timeout 300 --timeout-method thread > $OUT/ab_${name}_pytest.log 2>&1 || { tail -30 $OUT/ab_${name}_pytest.log; exit 1; }
tail -1 $OUT/ab_${name}_pytest.log
for r in 1 2; do
  QPGPU_LIB=$lib timeout -k 10 600 python bench.py --full --cpu-sample 0 --steps 10 > $OUT/ab_${name}_$r.log 2>&1 || exit 1
  echo "$name $r: $(grep -o '"value": [0-9.]*\|"quotient_avg_launch_ms": [0-9.]*' $OUT/ab_${name}_$r.log | head -2 | tr '\n' ' ')"
  timeout -k 10 600 python bench.py --full --cpu-sample 0 --steps 10 > $OUT/ab_base_$r.log 2>&1 || exit 1
  echo "base $r: $(grep -o '"value": [0-9.]*\|"quotient_avg_launch_ms": [0-9.]*' $OUT/ab_base_$r.log | head -2 | tr '\n' ' ')"
done
