#!/bin/bash
# Build a kernel-variant library for a same-box A/B: ONE object of csrc/Makefile recompiled with extra -D switches, linked
# with the tree's other objects (run `make -C pl-nerf_amd/csrc` first), written to tools/_head/lib<name>.so (git-ignored).
# The compile line is the Makefile's own (`make -n -B <object>`), so the flags -- and the register-resident forward's
# -amdgpu-mfma-vgpr-form -- are written there alone.
#   bash tools/build_variant.sh rrPFD3 mlp_rr_i_f16_2_1_0.o "-DRR_PFD=3"
#   bash tools/ab.sh "default lib:rrPFD3"
# With -DRR_SINGLE_TU among the switches (the object is mlp_rr.o or mlp_rr_bf16.o: every instantiation of that element type
# in one translation unit, which the trace hooks need) that element's per-instantiation objects stay out of the link:
#   bash tools/build_variant.sh rrtrace mlp_rr.o "-DRR_SINGLE_TU -DRR_TRACE=100"      (read by tools/trace_rr.py)
#   bash tools/build_variant.sh rrreport mlp_rr.o "-DRR_SINGLE_TU"                    (resource report of all six half kernels)
# (how profiles/r05_forward_knobs_ab.txt and r05_dgrad_prefetch_ab.txt were made)
set -e
name=$1; obj=$2; defs=$3
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R/pl-nerf_amd/csrc
tmp=$(mktemp -d); var=$tmp/variant_$name.o
compile=$(make -n -B $obj | grep -- " -o $obj\$")
[ -n "$compile" ] || { echo "$obj: no object of csrc/Makefile"; exit 1; }
mkdir -p $R/tools/_head
${compile% -o $obj} -w $defs -o $var -Rpass-analysis=kernel-resource-usage 2> $tmp/err || { tail -5 $tmp/err; exit 1; }
skip="^$obj\$"
case "$defs" in *RR_SINGLE_TU*) case $obj in mlp_rr.o) skip="$skip|^mlp_rr_i_f16_";; mlp_rr_bf16.o) skip="$skip|^mlp_rr_i_bf16_";; esac;; esac
objs=$(make -s print-objs | tr ' ' '\n' | grep -v -E "$skip" | tr '\n' ' ')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o $R/tools/_head/lib$name.so $objs $var
grep -E "Function Name|VGPRs:|VGPRs Spill|ScratchSize" $tmp/err | paste - - - - | sed 's/\[-Rpass-analysis=kernel-resource-usage\]//g; s/[^ ]*: remark: //g' | cut -c1-220 | head -16
rm -rf $tmp
echo "built tools/_head/lib$name.so"
