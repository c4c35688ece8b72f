#!/bin/bash
# run the contact bench once per tools/_ab/lib_*.so (pass names as arguments)
mkdir -p gpurun_out
for v in "$@"; do
  BOUT=${BENCH_OUT:-bench_out}; mkdir -p $BOUT
  SOARM_SIM_LIB=tools/_ab/lib_$v.so timeout -k 10 300 python bench.py --full --no-cpu-baseline > $BOUT/ab_$v.json 2> $BOUT/ab_$v.err || exit $?
  python -c "import json,sys; d=json.loads(open('$BOUT/ab_$v.json').read().strip().split(chr(10))[-1]); print('$v', round(d['value']), d['roofline']['kernel_ms_per_step'])"
done
