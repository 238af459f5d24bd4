# The C++ programs of the ICP tests, with the flags of this directory's Makefile:  make -C tests/cpp -f icp.mk [target]
#   _build/icp_snippet      the C++ caller of include/ouster/algorithm/align_clouds.h (tests/test_icp_api_cpu.py builds it the same way)
#   _build/icp_batch_tool   hip::DeviceFrameBatch::align_voxels (tests/test_gpu_icp_batch.py)
#   _build/icp_lanes        the grid and correspondence kernels' source on the CPU, one thread per lane (tests/test_icp_lanes_cpu.py)
#   icp_ref_sanitized       the host half alone (csrc/host/icp_util.cpp, pose_util.cpp) under ASan / UBSan, built and run: no GPU,
#                           no library
ROOT := ../..
CXX ?= g++
ROCM ?= /opt/rocm
CSRC := $(ROOT)/ouster_sdk_amd/csrc
CXXFLAGS := -O1 -g -std=c++17 -Wall -Wextra -I$(ROOT)/include -I$(ROCM)/include -D__HIP_PLATFORM_AMD__
LIBS := -L$(ROOT)/ouster_sdk_amd/lib -louster_core_amd -louster_hip -L$(ROCM)/lib -lamdhip64 \
        -Wl,-rpath,'$$ORIGIN/../../../ouster_sdk_amd/lib' -Wl,-rpath,$(ROCM)/lib

all: _build/icp_snippet _build/icp_batch_tool _build/icp_lanes icp_ref_sanitized

_build/icp_snippet: icp_snippet.cpp $(ROOT)/include/ouster/algorithm/align_clouds.h $(ROOT)/ouster_sdk_amd/lib/libouster_core_amd.so
	mkdir -p _build
	$(CXX) $(CXXFLAGS) -Werror -o $@ icp_snippet.cpp $(LIBS)

_build/icp_batch_tool: icp_batch_tool.cpp $(wildcard $(ROOT)/include/ouster/hip/*.h) $(ROOT)/ouster_sdk_amd/lib/libouster_core_amd.so
	mkdir -p _build
	$(CXX) $(CXXFLAGS) -o $@ icp_batch_tool.cpp $(LIBS)

_build/icp_lanes: icp_lanes.cpp $(CSRC)/k_icp.hip $(CSRC)/k_icp.h $(CSRC)/k_voxel.hip $(CSRC)/voxel_dev.h host_lanes/hip/hip_runtime.h
	mkdir -p _build
	$(CXX) -O1 -std=c++20 -ffp-contract=off -pthread -Ihost_lanes -I. -I$(ROOT)/include -o $@ icp_lanes.cpp

icp_ref_sanitized: icp_ref_main.cpp $(CSRC)/host/icp_util.cpp $(CSRC)/host/pose_util.cpp $(CSRC)/icp_host.h
	mkdir -p _build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o _build/icp_ref_sanitized icp_ref_main.cpp $(CSRC)/host/icp_util.cpp $(CSRC)/host/pose_util.cpp
	_build/icp_ref_sanitized

.PHONY: all icp_ref_sanitized
