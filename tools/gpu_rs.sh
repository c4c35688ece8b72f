#!/bin/bash
# row-space PGS iteration: parity diagnostic (RS and quad kernels vs the oracle), then the contact
# bench with the RS kernel and with the quad kernel (steady window and the driver's window)
mkdir -p gpurun_out
timeout -k 10 300 python tools/rs_check.py ${N:-2048} > gpurun_out/rs_check.log 2>&1; rc=$?
cat gpurun_out/rs_check.log
if [ $rc -ne 0 ]; then exit $rc; fi
for w in 1 0; do
  BOUT=${BENCH_OUT:-bench_out}; mkdir -p $BOUT
  SOARM_RS=$w timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-other-solver > $BOUT/bench_rs$w.json 2> $BOUT/bench_rs$w.err || exit $?
  SOARM_RS=$w timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-other-solver --no-steady --steps 20 --warmup 5 > $BOUT/benchd_rs$w.json 2>> $BOUT/bench_rs$w.err || exit $?
  python -c "import json; d=json.loads(open('$BOUT/bench_rs$w.json').read().strip().split(chr(10))[-1]); e=json.loads(open('$BOUT/benchd_rs$w.json').read().strip().split(chr(10))[-1]); print('rs=$w', 'steady', round(d['value']), {k: round(x,4) for k,x in d['roofline']['kernel_ms_per_step'].items()}, 'driver', round(e['value']), {k: round(x,4) for k,x in e['roofline']['kernel_ms_per_step'].items()})"
done
