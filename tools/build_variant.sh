#!/bin/bash
# Build container: a variant of libpsg.so with ONE translation unit recompiled with extra flags, for A/B probes:
#   tools/build_variant.sh NAME psg_resgcn "-DEBG_STOP=1"   ->  build/libpsg_NAME.so   (git-ignored)
# The other objects are the ones `make` built, by the Makefile's own list (print-objs): the variant exports what libpsg.so exports.
# ResGCN is two units: psg_resgcn (model, forward, backward and - through psg_resgcn_kernels.cuh - every kernel, so the kernel
# switches EBG_* and PSG_GEMM_LEGACY_ORDER go here) and psg_resgcn_attack (the NB loop and the NU windows, host code only).
set -e
name=$1; unit=$2; flags=$3
cd "$(dirname "$0")/../pointsecguard_amd/csrc"
mkdir -p ../../build
cmd=$(make -n -B $unit.o | grep hipcc | head -1)
cmd=${cmd/ -c / $flags -c }
cmd=${cmd/-o $unit.o/-o ..\/..\/build\/${unit}_$name.o}
eval "$cmd"
objs=""
for o in $(make -s print-objs); do
  if [ $o = $unit.o ]; then objs="$objs ../../build/${unit}_$name.o"; else objs="$objs $o"; fi
done
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o ../../build/libpsg_$name.so $objs
echo built build/libpsg_$name.so
