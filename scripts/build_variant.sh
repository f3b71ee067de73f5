#!/bin/bash
# Build lidar_snow_sim_amd/_variants/libsnowgpu_<name>.so: the translation units named in SG_VARIANT_UNITS compiled with extra -D flags,
# the other translation units of build.SOURCES as they are (same-box A/B runs copy a variant over libsnowgpu.so on the GPU side, or load
# it beside the library in one process).  Without SG_VARIANT_UNITS: snowgpu_kernels.hip (the per-beam kernels and their tunables) and
# snowgpu_api.cpp (table registration: the shape of the step-major range index it files, sg_range_index.h).
# usage: [SG_VARIANT_UNITS="snowgpu_box.hip"] scripts/build_variant.sh <name> [-DX=1 ...]
set -e
cd "$(dirname "$0")/.."
N=$1; shift
UNITS=${SG_VARIANT_UNITS:-"snowgpu_kernels.hip snowgpu_api.cpp"}
C=lidar_snow_sim_amd/csrc; V=lidar_snow_sim_amd/_variants; mkdir -p $V $C/_obj
python -m lidar_snow_sim_amd.build > /dev/null
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function"
OBJS=""; PIDS=""
for U in $UNITS; do
    O=$C/_obj/${U%.*}_$N.o
    hipcc $F "$@" -x hip -c $C/$U -o $O &
    PIDS="$PIDS $!"; OBJS="$OBJS $O"
done
for P in $PIDS; do wait $P; done
OTHERS=$(python -c "from lidar_snow_sim_amd.build import SOURCES; print(' '.join('$C/_obj/' + s.rsplit('.', 1)[0] + '.o' for s in SOURCES if s not in '$UNITS'.split()))")
hipcc --offload-arch=gfx950 -shared -fPIC -o $V/libsnowgpu_$N.so $OBJS $OTHERS -ldl
echo $V/libsnowgpu_$N.so
