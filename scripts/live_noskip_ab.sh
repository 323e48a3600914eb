# No loss where the backward has nothing to skip: rnnt_loss_simple forward + backward at the c3 shape on inputs scaled by
# 0.05 (a near-uniform model: ~0.89 of the 16x64 blocks live), this tree against a built checkout of the parent commit,
# interleaved.  Usage: bash scripts/live_noskip_ab.sh PARENT_TREE [PAIRS] [SCALE]
set -o pipefail
parent=$1; pairs=${2:-3}; scale=${3:-0.05}
for i in $(seq 1 $pairs); do
  timeout -k 10 120 python scripts/simple_step_time.py --scale $scale --root $parent --label parent || exit 1
  timeout -k 10 120 python scripts/simple_step_time.py --scale $scale --label change || exit 1
done
