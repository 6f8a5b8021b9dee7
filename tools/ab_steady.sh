#!/bin/bash
# A/B of the steady round on the GPU box: the driver's bench job (no extras), four sides alternating --
#   parent   ropebwt2_amd/lib/librb2hip_<tag>.so (the parent commit's library: tools/build_variant.sh in a checkout of it)
#   off      the working tree's library with RB2_STEADY=0 (the report is read and the run-ahead bound holds; the launches are the parent's)
#   tree     the working tree's library
#   nobound  the working tree's library with RB2_STEADY_AHEAD=0 (no bound: the host hears as late as it queues ahead)
# value + per-kernel-group milliseconds per step (hipEvent scopes).   usage: ab_steady.sh <tag> [steps] [repeats]
TAG=$1; STEPS=${2:-20}; REP=${3:-3}
cd $(dirname $0)/..
one() { python bench.py --steps $STEPS --warmup 2 --full --no-extras --no-cpu-baseline 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.readline()); n=d.get('kernels_ms_steps', d['steps'])
print('$1', round(d['value'],3), 'counts_ok', d['config'].get('counts_ok'), {k: round(v/n,2) for k,v in d['kernels_ms'].items() if v})"; }
for i in $(seq $REP); do
  RB2_HIP_LIB=$PWD/ropebwt2_amd/lib/librb2hip_$TAG.so one parent
  RB2_STEADY=0 one off
  one tree
  RB2_STEADY_AHEAD=0 one nobound
done
