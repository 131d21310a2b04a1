#!/bin/bash
# Builds a variant of the library for interleaved A/B runs:  bash tools/build_variant.sh NAME [-DMACRO=value ...]
# -> skelsplat_amd/ab_NAME.so (git-ignored, but it travels to the GPU box); use with SKS_LIB_OVERRIDE=skelsplat_amd/ab_NAME.so
# SKS_VARIANT_CSRC=<dir>: compile that copy of csrc/ instead (e.g. the parent commit's: `git archive <commit> skelsplat_amd/csrc include`
# unpacked into a scratch directory -- the sources include ../../include/skelsplat_hip.h, so include/ must lie beside skelsplat_amd/ there too)
root=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
cd "${SKS_VARIANT_CSRC:-$root/skelsplat_amd/csrc}" || exit 1
F="-O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -Wno-unused-function -mllvm -disable-machine-sink"
tmp=$(mktemp -d)
# (the sources and flags of skelsplat_amd/build.py)
for s in sks_raster sks_ops sks_loop sks_triangulate sks_keypoint sks_fuse sks_report; do /opt/rocm/bin/hipcc $F "$@" -c -o $tmp/$s.o $s.hip & done
/opt/rocm/bin/hipcc $F -fno-slp-vectorize "$@" -c -o $tmp/sks_ssim.o sks_ssim.hip &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared -o "$root/skelsplat_amd/ab_$name.so" $tmp/*.o && echo "built skelsplat_amd/ab_$name.so"
rm -rf $tmp
