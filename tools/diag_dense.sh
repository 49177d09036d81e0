#!/bin/bash
# Diagnostic builds of the library (results of a cut build are garbage; the timing is what is read):
#   tools/diag_dense.sh pN      dense block's panel loop cut after N <= 12 panels (the in-wave finish of the last 16 pivots still runs) -> tools/diaglib/libdiag_pN.so
#   tools/diag_dense.sh stamps  cycle stamps inside dense_lu, its tile steps and dense_finish (tools/diag_dense_stamps.py reads them) -> libdiag_stamps.so
#   tools/diag_dense.sh stampsN the same with MISTRA_DENSE_TILE_FROM=N (3: panels only, the form before the tile steps) -> libdiag_stampsN.so
cd "$(dirname "$0")/.."
mkdir -p tools/diaglib
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math"
for V in "$@"; do
  if [ "${V%[0-3]}" = env ]; then      # the schedule compiler's A/B switches (MISTRA_DIAG_*), read from the environment -> libdiag_env.so; envN: with the kernels of MISTRA_DENSE_TILE_FROM=N -> libdiag_envN.so
    KOBJ=mistra_amd/build/ros3_kernel.o
    if [ "$V" != env ]; then
      KOBJ=/tmp/ros3_kernel_$V.o
      hipcc --offload-arch=gfx950 $FLAGS -DMISTRA_DENSE_TILE_FROM=${V#env} -c mistra_amd/csrc/ros3_kernel.hip -o $KOBJ || exit 1
    fi
    hipcc --offload-arch=gfx950 $FLAGS -DMISTRA_DIAG_ENV -DMISTRA_USER_MECHS=0 -c mistra_amd/csrc/capi.cpp -o /tmp/capi_env.o &&
    hipcc --offload-arch=gfx950 $FLAGS -DMISTRA_DIAG_ENV -c mistra_amd/csrc/schedule.cpp -o /tmp/schedule_env.o &&
    hipcc --offload-arch=gfx950 -shared -fPIC -o tools/diaglib/libdiag_$V.so $KOBJ /tmp/capi_env.o /tmp/schedule_env.o mistra_amd/build/mech_tables.o mistra_amd/build/rates.o mistra_amd/build/pack.o mistra_amd/build/ros_unit_*.o -ldl
    continue
  fi
  case $V in
    p*) DEF="-DMISTRA_DIAG_DENSE_PANELS=${V#p}";;
    stamps) DEF="-DMISTRA_DIAG_STAMPS";;
    stamps[0-3]) DEF="-DMISTRA_DIAG_STAMPS -DMISTRA_DENSE_TILE_FROM=${V#stamps}";;
  esac
  hipcc --offload-arch=gfx950 $FLAGS $DEF -c mistra_amd/csrc/ros3_kernel.hip -o /tmp/ros3_diag_$V.o &&
  hipcc --offload-arch=gfx950 -shared -fPIC -o tools/diaglib/libdiag_$V.so /tmp/ros3_diag_$V.o mistra_amd/build/capi.o mistra_amd/build/schedule.o mistra_amd/build/mech_tables.o mistra_amd/build/rates.o mistra_amd/build/pack.o mistra_amd/build/ros_unit_*.o mistra_amd/build/ros_user_*.o -ldl
done
