#!/bin/bash
# A/B of the forked round ("the forked round") on the GPU box: the driver's bench job (no extras), the sides alternating --
#   parent   ropebwt2_amd/lib/librb2hip_<tag>.so (the parent commit's library: tools/build_variant.sh in a checkout of it)
#   fork0    the working tree's library with RB2_LEAN_FORK=0 (one stream: the parent's launches; k_part and k_tfix as they were)
#   tree     the working tree's library as it comes (whichever setting is the default)
# value + per-kernel-group milliseconds per step (hipEvent scopes; with the fork on, k_sym and k_tscan of a forked round are timed on the side stream and
# the groups no longer add up to the wall time); one run of the tree in front of the repeats is printed and discarded.
#   usage: ab_lean_fork.sh <tag> [steps] [repeats]
set -o pipefail
TAG=$1; STEPS=${2:-20}; REP=${3:-3}
cd $(dirname $0)/..
one() { timeout -k 10 300 python bench.py --steps $STEPS --warmup 2 --full --no-extras --no-cpu-baseline 2>/dev/null | tail -1 | python -c "
import json,sys
d=json.loads(sys.stdin.readline()); n=d.get('kernels_ms_steps', d['steps'])
print('$1', round(d['value'],3), 'counts_ok', d['config'].get('counts_ok'), {k: round(v/n,2) for k,v in d['kernels_ms'].items() if v})" || exit 1; }
one warmup-discarded   # (the first bench run on a box that sat idle runs at other clocks than the ones behind it: not a side)
for i in $(seq $REP); do
  RB2_HIP_LIB=$PWD/ropebwt2_amd/lib/librb2hip_$TAG.so one parent
  RB2_LEAN_FORK=0 one fork0
  one tree
done
exit 0
