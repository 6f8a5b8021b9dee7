#!/bin/bash
# A/B of the lean round on the GPU box: the driver's bench job (no extras), the sides alternating --
#   parent   ropebwt2_amd/lib/librb2hip_<tag>.so (the parent commit's library: tools/build_variant.sh in a checkout of it)
#   lean0    the working tree's library with RB2_STEADY_LEAN=0 (the launches are the parent's)
#   tree     the working tree's library (no INS_E / INS_A in steady dense rounds, k_part and k_merge read L and A)
#   <extra>  optional: ropebwt2_amd/lib/librb2hip_<extra>.so with RB2_STEADY_LEAN=2 (a build that still has the second stage: k_sym reads A only)
# value + per-kernel-group milliseconds per step (hipEvent scopes).   usage: ab_lean.sh <tag> [steps] [repeats] [extra]
set -o pipefail
TAG=$1; STEPS=${2:-20}; REP=${3:-3}; EXTRA=${4:-}
cd $(dirname $0)/..
one() { timeout -k 10 300 python bench.py --steps $STEPS --warmup 2 --full --no-extras --no-cpu-baseline 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.readline()); n=d.get('kernels_ms_steps', d['steps'])
print('$1', round(d['value'],3), 'counts_ok', d['config'].get('counts_ok'), {k: round(v/n,2) for k,v in d['kernels_ms'].items() if v})" || exit 1; }
for i in $(seq $REP); do
  RB2_HIP_LIB=$PWD/ropebwt2_amd/lib/librb2hip_$TAG.so one parent
  RB2_STEADY_LEAN=0 one lean0
  one tree
  [ -n "$EXTRA" ] && RB2_STEADY_LEAN=2 RB2_HIP_LIB=$PWD/ropebwt2_amd/lib/librb2hip_$EXTRA.so one $EXTRA
done
exit 0
