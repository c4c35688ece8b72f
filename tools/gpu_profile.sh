#!/bin/bash
# One GPU session for the round's evidence: gpu tests, smoke, bench lines (contact with CPU
# baseline, nocontact, dr, rollout, mpc), and for the headline (contact) and the Koopman-MPC
# config the rocprofv3 kernel-trace summary of the bench command plus separate PMC passes
# (FETCH_SIZE, WRITE_SIZE, SQ instruction/wait counters) on the hot kernels.
# Every GPU step has its own time limit; a failure or timeout ends the script.
#   usage: tools/gpu_profile.sh [tag] [--no-tests]   (PART=bench | PART=prof: only that half)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-r02}
O=$R/gpurun_out
mkdir -p $O
export TMPDIR=/tmp
step() {  # name, limit, command...
  local name=$1 lim=$2; shift 2
  echo "== $name" >&2
  timeout -k 10 $lim "$@"
  local rc=$?
  echo "== $name rc=$rc" >&2
  if [ $rc -ne 0 ]; then exit $rc; fi
}
if [ "$2" != "--no-tests" ] && [ "$PART" != "prof" ]; then
  step pytest 600 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread > $O/pytest_gpu.log 2>&1
  tail -2 $O/pytest_gpu.log
  step smoke 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
fi
if [ "$PART" != "prof" ]; then
step bench_contact 600 python bench.py --full > $O/bench_contact.json 2> $O/bench_contact.err
step bench_contact_newton 600 python bench.py --full --solver newton --no-cpu-baseline > $O/bench_contact_newton.json 2> $O/bench_contact_newton.err
step bench_driver 300 python bench.py --full --steps 20 --warmup 5 > $O/bench_contact_steps20_warmup5.json 2> $O/bench_contact_drv.err
step bench_nocontact 300 python bench.py --full --config nocontact --steps 200 --warmup 20 --cpu-seconds 8 > $O/bench_nocontact.json 2> $O/bench_nocontact.err
step bench_dr 600 python bench.py --full --config dr --steps 50 --warmup 5 --cpu-seconds 8 > $O/bench_dr.json 2> $O/bench_dr.err
step bench_rollout 600 python bench.py --full --config rollout --steps 100 --warmup 5 --cpu-seconds 8 > $O/bench_rollout.json 2> $O/bench_rollout.err
step bench_mpc 600 python bench.py --full --config mpc --cpu-seconds 8 > $O/bench_mpc.json 2> $O/bench_mpc.err
step bench_mpc_dbkn 600 python bench.py --full --config mpc_dbkn --steps 30 --warmup 5 --cpu-seconds 8 > $O/bench_mpc_dbkn.json 2> $O/bench_mpc_dbkn.err
step bench_plumbing 300 python bench.py --full --config plumbing > $O/bench_plumbing.json 2> $O/bench_plumbing.err
fi
[ "$PART" = "bench" ] && exit 0
# the multi-rank path with real kernels: 2 self-launched ranks sharing the box's one GPU (gloo)
step bench_gloo2 300 python bench.py --full --gpus 2 --dist-backend gloo --steps 10 --warmup 2 --no-cpu-baseline --no-steady --no-other-solver > $O/bench_gloo2.json 2> $O/bench_gloo2.err
KRE="k_substep|k_collide|k_step|k_geom|k_mpc_step|k_bias"
cd /tmp
for SPEC in contact:contact: contact_newton:contact:--solver_newton mpc:mpc:; do
  IFS=: read TAGC C EXTRA <<< "$SPEC"
  EXTRA=${EXTRA//_/ }
  P=$O/prof_${TAG}_$TAGC
  step trace_$TAGC 600 rocprofv3 --kernel-trace --stats -f csv -d $P -o trace -- python3 $R/bench.py --full --config $C $EXTRA --no-cpu-baseline > $O/bench_${TAGC}_traced.json
  NP="--steps 10 --warmup 2 --no-cpu-baseline --no-profile --no-steady --no-other-solver"
  step pmc_fetch_$TAGC 300 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex "$KRE" -f csv -d $P -o pmc_fetch -- python3 $R/bench.py --config $C $EXTRA $NP
  step pmc_write_$TAGC 300 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex "$KRE" -f csv -d $P -o pmc_write -- python3 $R/bench.py --config $C $EXTRA $NP
  step pmc_sq_$TAGC 300 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY --kernel-include-regex "$KRE" -f csv -d $P -o pmc_sq -- python3 $R/bench.py --config $C $EXTRA $NP
done
ls -R $O/prof_${TAG}_contact | head -20
