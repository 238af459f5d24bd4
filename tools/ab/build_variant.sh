#!/bin/bash
# Experiment build of the HIP library with extra compiler flags -> tools/ab/libouster_hip_<name>.so (for ab_inproc.py).
#   tools/ab/build_variant.sh maxilp -mllvm -amdgpu-sched-strategy=max-ilp
# Run where hipcc is (the build container); the .so travels with the snapshot.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../.."
B=/tmp/ouster_variant_$NAME; mkdir -p $B
F="--offload-arch=gfx950 -O3 -std=c++20 -fPIC -Wno-unused-result $*"
C=ouster_sdk_amd/csrc
for i in 0 1 2 3 4 5; do hipcc $F -DOUSTER_SPEC_ID=$i -c -o $B/k_decode_$i.o $C/k_decode.hip & done
for i in 1 2 3 4 5; do hipcc $F -DOUSTER_SPEC_ID=$i -c -o $B/k_decode_stream_$i.o $C/k_decode_stream.hip & done
FEATURES="image frame_ops pose normals voxel icp"
STANDALONE="destagger cartesian dewarp osf"   # the Makefile's; the frame dewarp's experimental kernels only with -DOUSTER_EXPERIMENTS
case " $* " in *" -DOUSTER_EXPERIMENTS "*) EXP=k_dewarp_experiments ;; *) EXP= ;; esac
for s in $(printf 'k_%s ' $STANDALONE) $EXP decode_launch ouster_hip_capi host_pool $(printf 'capi_%s ' $STANDALONE $FEATURES); do hipcc $F -c -o $B/$s.o $C/$s.hip & done
for s in $FEATURES; do hipcc $F -ffp-contract=off -c -o $B/k_$s.o $C/k_$s.hip & done   # the Makefile's NO_CONTRACT
for s in decode_plan standalone_plan; do hipcc $F -x hip -c -o $B/$s.o $C/$s.cpp & done
for s in pose normals voxel icp; do ${CXX:-g++} -O2 -std=c++17 -fPIC -ffp-contract=off -c -o $B/${s}_util.o $C/host/${s}_util.cpp & done
wait
hipcc $F -shared -o tools/ab/libouster_hip_$NAME.so $B/*.o
ls -la tools/ab/libouster_hip_$NAME.so
