#!/bin/bash
# Build a trace variant of the library (mlp_h16.o recompiled with -DPLNERF_TRACE=<block> by tools/build_variant.sh, linked
# with every other product object -- run `make -C pl-nerf_amd/csrc` first) and print the phase breakdown of the ping-pong
# forward kernel (BWD=1: of the dgrad kernel).  Needs hipcc and a GPU.
export PLNERF_ALLOW_TOOLS_BUILD=1      # variant libraries carry ablation / trace switches (pl-nerf_amd/_lib.py refuses them otherwise)
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
bash $R/tools/build_variant.sh trace mlp_h16.o "-DPLNERF_TRACE=${TRACE_BLOCK:-3000} ${EXTRA_DEFS}"
out=$R/tools/_head/libtrace.so
if [ -n "$BWD" ]; then PLNERF_HIP_LIB=$out python $R/tools/trace_bwd.py; exit 0; fi
for p in ${PRECS:-bf16 bf16x3}; do
  for m in ${MODES:-inference train}; do PLNERF_FWD_KERNEL=pp PLNERF_HIP_LIB=$out python $R/tools/trace_fwd.py $p $m; done
done
