#!/bin/bash
# build rmsc03-only libmxa variants: NAME:SRCROOT:FLAGS...   (SRCROOT "." = working tree)
# FLAGS are the per-configuration masks and the capacities of mxa_config.h / mxa_kernels.hip, and
# -DMXA_ONLY_CFG=<id> for a configuration other than rmsc03 (id 0), for example:
#   "b:.:"                                                   the shipped build
#   "q:.:-DMXA_INPLACE_MASK=0"                               every exchange round trip through the queue
#   "w:.:-DMXA_TEMPER_FILL_MASK=0 -DMXA_ONE_ADVANCE_MASK=0"  state words in the stream windows
#   "t:.:-DMXA_VARIATE_O_MASK=0 -DMXA_VARIATE_AGENT_MASK=0"  serial draws, no variate tables
#   "p:/path/to/a/checkout:"                                 another source tree (an A/B parent)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
pids=()
for spec in "$@"; do
  IFS=: read name root flags <<< "$spec"
  [ "$root" = "." ] && root=$R
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++20 -ffp-contract=off -fno-fast-math -fPIC -shared \
    -Wno-unused-result -Wno-unused-value -mllvm -structurizecfg-skip-uniform-regions -DMXA_ONLY_RMSC03 $flags -I$root/marl-optimal-execution_amd/csrc -I$root/include \
    $root/marl-optimal-execution_amd/csrc/mxa_api.hip -o $R/marl-optimal-execution_amd/lib/libmxa_$name.so &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
