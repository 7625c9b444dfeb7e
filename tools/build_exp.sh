#!/bin/bash
# Build an experiment variant of libtd3hip.so into tools/exp/ (not product code).
#   tools/build_exp.sh NAME "-DSOME_KNOB=1 ..."   ->  tools/exp/libtd3hip_NAME.so
# Knockout builds (-DTD3_KO_* / -DTD3_X_*: wrong results, timing only) compile kernels.hip with
# tools/exp_patches/knockout.patch applied to a scratch copy: the product source holds no
# wrong-result blocks.  (knockout.patch is a record against kernels.hip as one file, before its split into the
# csrc/kernels_*.h parts; it no longer applies.)
set -e
cd "$(dirname "$0")/.."
out=${EXP_DIR:-tools/exp}; mkdir -p $out
name=$1; flags=${2:-}
src=td3_amd/csrc
# Store-policy builds (TD3_STORE_POLICY / TD3_STATE_STORE / TD3_PARAM_STORE) compile every source
# against dev.h with tools/exp_patches/store_policy.patch applied: the product's dev.h has plain
# stores only.
if [[ "$flags" == *TD3_KO_* || "$flags" == *TD3_X_* || "$flags" == *TD3_STORE_POLICY* || "$flags" == *TD3_STATE_STORE* || \
      "$flags" == *TD3_PARAM_STORE* ]]; then
  scratch=$(mktemp -d)
  mkdir -p "$scratch/td3_amd/csrc" "$scratch/include"          # the sources' relative includes
  cp td3_amd/csrc/*.h td3_amd/csrc/*.hip "$scratch/td3_amd/csrc"/
  cp include/*.h "$scratch/include"/
  src=$scratch/td3_amd/csrc
  if [[ "$flags" == *TD3_KO_* || "$flags" == *TD3_X_* ]]; then patch -s "$src/kernels.hip" tools/exp_patches/knockout.patch; fi
  if [[ "$flags" == *STORE* ]]; then patch -s "$src/dev.h" tools/exp_patches/store_policy.patch; fi
fi
# the product's own source list (td3_amd/build.py SOURCES: csrc/NAME.hip), taken from $src
sources=$(python3 -c 'from td3_amd.build import SOURCES; print(" ".join(SOURCES))')
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -shared -ffp-contract=off -mllvm -amdgpu-kernarg-preload-count=6 $flags \
  $(for f in $sources; do echo "$src/${f#csrc/}"; done) \
  -o $out/libtd3hip_$name.so -lrccl
ls -la $out/libtd3hip_$name.so
