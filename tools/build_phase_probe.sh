#!/bin/bash
# Build a library variant with wall-clock / shader-clock stamps around the kernel phases for the phase probes (the kernels carry their stamps as macros):
#   tools/build_phase_probe.sh dp_wave|nn|epilogue   ->  gpurun_variants/libvaeq_<name>prof.so
#   VAEQ_LIB=$PWD/gpurun_variants/libvaeq_<name>prof.so python tools/probe_{dp,nn,epi}_phases.py        (on the GPU box)
# Only the unit that holds the stamped kernel is recompiled (tools/build_variant.sh: the others come from vae_equalizer_amd/_obj).
set -e
ROOT=$(cd $(dirname $0)/.. && pwd); C=$ROOT/vae_equalizer_amd/csrc
case $1 in
  dp_wave) f=vaeq_dp_wave.hip; X="-DVAEQ_PHASE_STAMPS";;
  nn) f=vaeq_nn.hip; X="-DVAEQ_NN_STAMPS -DVAEQ_NN_HALF_STAMPS";;
  epilogue) f=vaeq_epilogue.hip; X="-DVAEQ_EPI_STAMPS";;
  *) echo "dp_wave|nn|epilogue"; exit 1;;
esac
HIPFLAGS="$X" $ROOT/tools/build_variant.sh $1prof $C/$f
