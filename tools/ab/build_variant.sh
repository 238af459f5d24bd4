#!/bin/bash
# Experiment build of the HIP library with extra compiler flags -> tools/ab/libouster_hip_<name>.so (for ab_inproc.py).
#   tools/ab/build_variant.sh maxilp -mllvm -amdgpu-sched-strategy=max-ilp
# The Makefile's own recipe with its objects and library in a scratch directory (a -DOUSTER_EXPERIMENTS among the flags is
# EXPERIMENTS=1).  Run where hipcc is (the build container); the .so travels with the snapshot.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../.."
B=/tmp/ouster_variant_$NAME
make -j"${JOBS:-$(nproc)}" OBJ=$B LIB=$B EXTRA_HIPFLAGS="$*" $B/libouster_hip.so
cp $B/libouster_hip.so tools/ab/libouster_hip_$NAME.so
ls -la tools/ab/libouster_hip_$NAME.so
