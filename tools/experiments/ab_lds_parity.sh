#!/usr/bin/env bash
# A/B of library variants under densepoints_amd/lib/ (VARIANTS; default: the
# default library alone), each through bench.py's parity headline only; prints
# rate, E and the time per evaluation.  Alternated twice.  Written for the
# parity-kernel LDS-staging study, whose diagnostic
# variants were built from r05_parity_lds_tiles.patch; that patch applies to
# dp_kernels.hip as of commit 35620e7, before it became dp_refine.hip.
set -u
cd "$(dirname "$0")/../.."
mkdir -p gpurun_out
for rep in ${REPS:-1 2}; do
for v in ${VARIANTS:-libdensepoints.so}; do
  DP_LIB_VARIANT=$v timeout -k 10 300 python -u bench.py --no-fast --no-densify --no-seeds --no-cpu --steps 3 \
    > gpurun_out/abl_${v}_$rep.log 2>&1; rc=$?
  [ $rc -eq 0 ] || { echo "$v rc=$rc"; tail -5 gpurun_out/abl_${v}_$rep.log; exit $rc; }
  tail -1 gpurun_out/abl_${v}_$rep.log | python3 -c "
import json,sys
d=json.loads(sys.stdin.read())
B=d['config']['batch_per_gpu']
print('$v', 'rep', $rep, 'Mpatches/s', d['value'], 'E', d['E_mean_evals_per_patch'], 'kernel_ms', d['kernel_ms_per_launch'],
      'ns_per_eval', round(d['kernel_ms_per_launch'] * 1e6 / (d['E_mean_evals_per_patch'] * B), 3))"
done
done
