#!/bin/bash
# A/B of the window directory ("the window directory") on the GPU box: the driver's bench job (no extras), the sides alternating --
#   parent   ropebwt2_amd/lib/librb2hip_<tag>.so (the parent commit's library: tools/build_variant.sh in a checkout of it)
#   dir0     the working tree's library with RB2_LEAN_DIR=0 (the per-leaf directory in every round: the parent's launches)
#   tree     the working tree's library as it comes (whichever setting is the default)
# value + per-kernel-group milliseconds per step (hipEvent scopes; k_sym and k_tscan of a forked round are timed on the side stream, so the groups do not
# add up to the wall time); one run of the tree in front of the repeats is printed and discarded.
#   usage: ab_lean_dir.sh <tag> [steps] [repeats]
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
  RB2_LEAN_DIR=0 one dir0
  one tree
done
exit 0
