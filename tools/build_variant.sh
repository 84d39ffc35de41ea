#!/bin/bash
# build_variant.sh NAME "-DFOO=1 ..." ["ring-unit flags"] : libdrrt_hip variant with extra defines
#   -> adjointnonlinearraytracing_amd/csrc/_variants/NAME.so
# (same-box A/B runs: DRRT_HIP_LIB=.../NAME.so python bench.py ..., tools/ab_variants.sh).  The third argument replaces the
# ring-window unit's scheduling option (default: the Makefile's -mllvm -amdgpu-sched-strategy=max-ilp).
# Every unit of the Makefile's SRCS is compiled (a library that misses one does not load).
set -e
cd "$(dirname "$0")/../adjointnonlinearraytracing_amd/csrc"
N=$1; D=$2; RF=${3--mllvm -amdgpu-sched-strategy=max-ilp}
FL="-O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -mllvm -disable-vector-combine --offload-arch=gfx950 -fvisibility=hidden -Wno-unused-function"
UNITS=$(sed -n 's/^SRCS *= *//p' Makefile | sed 's/\.hip//g')
mkdir -p _variants/_o_$N
for f in $UNITS; do
  if [ $f = drrt_adjoint_ring ]; then /opt/rocm/bin/hipcc $FL $RF $D -c $f.hip -o _variants/_o_$N/$f.o &
  else /opt/rocm/bin/hipcc $FL $D -DDRRT_SRC_ID=\"variant:$N\" -c $f.hip -o _variants/_o_$N/$f.o & fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o _variants/$N.so _variants/_o_$N/*.o
rm -rf _variants/_o_$N
echo built _variants/$N.so
