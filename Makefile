# Builds everything in-tree (the .so files travel to the GPU box with the snapshot):
#   ouster_sdk_amd/lib/libouster_hip.so        HIP kernels + C ABI (include/ouster_hip.h), gfx950
#   ouster_sdk_amd/lib/libouster_core_amd.so   C++ host API (include/ouster/core/*.h) over the C ABI
#   oracle/_build/libouster_oracle.so          CPU oracle (test infrastructure only)
HIPCC ?= hipcc
CXX ?= g++
LIB := ouster_sdk_amd/lib
CSRC := ouster_sdk_amd/csrc
# host/pose_util.cpp, host/normals_util.cpp, host/voxel_util.cpp, host/voxel_map_util.cpp, host/icp_util.cpp and host/registration_util.cpp
# are the plain C++ halves of interp_pose, normals, voxel down-sampling, the voxel map, ICP and ICPRegistration inside libouster_hip.so (objects of their own, below)
HOST_SRC := $(filter-out $(CSRC)/host/pose_util.cpp $(CSRC)/host/normals_util.cpp $(CSRC)/host/voxel_util.cpp $(CSRC)/host/voxel_map_util.cpp $(CSRC)/host/icp_util.cpp $(CSRC)/host/registration_util.cpp,$(wildcard $(CSRC)/host/*.cpp))
# EXPERIMENTS=1 also compiles the measured-slower kernel forms kept for A/B work (k_decode_wide_resolved, k_dwf_single, k_dwf_fused)
# EXTRA_HIPFLAGS: more compiler flags for a variant library (tools/ab/build_variant.sh, with OBJ= and LIB= of its own); a
# -DOUSTER_EXPERIMENTS among them is EXPERIMENTS=1
override EXPERIMENTS := $(strip $(EXPERIMENTS) $(filter -DOUSTER_EXPERIMENTS,$(EXTRA_HIPFLAGS)))
HIPFLAGS := --offload-arch=gfx950 -O3 -std=c++20 -fPIC -Wno-unused-result $(if $(EXPERIMENTS),-DOUSTER_EXPERIMENTS,)
HIPFLAGS += $(filter-out -DOUSTER_EXPERIMENTS,$(EXTRA_HIPFLAGS))
# the fused decode kernels are compiled once per packet-profile specialisation (parallel with -j)
OBJ := $(CSRC)/_build
SPEC_IDS := 0 1 2 3 4 5
STREAM_IDS := 1 2 3 4 5
FEATURES := image tonemap frame_ops pose normals voxel voxel_map icp registration
# the standalone calls of the hot path, k_<name>.hip + capi_<name>.hip each; contracted like the decode (they are not in NO_CONTRACT).
# k_dewarp_experiments.hip holds the frame dewarp's experimental kernels and is part of an EXPERIMENTS=1 build only.
STANDALONE := destagger cartesian dewarp osf
HIP_OBJS := $(foreach i,$(SPEC_IDS),$(OBJ)/k_decode_$(i).o) $(foreach i,$(STREAM_IDS),$(OBJ)/k_decode_stream_$(i).o) $(STANDALONE:%=$(OBJ)/k_%.o) $(if $(EXPERIMENTS),$(OBJ)/k_dewarp_experiments.o,) $(OBJ)/k_image.o $(OBJ)/k_tonemap.o $(OBJ)/k_frame_ops.o $(OBJ)/k_pose.o $(OBJ)/pose_util.o $(OBJ)/k_normals.o $(OBJ)/normals_util.o $(OBJ)/k_voxel.o $(OBJ)/voxel_util.o $(OBJ)/k_voxel_map.o $(OBJ)/voxel_map_util.o $(OBJ)/k_icp.o $(OBJ)/icp_util.o $(OBJ)/k_registration.o $(OBJ)/registration_util.o $(OBJ)/decode_launch.o $(OBJ)/decode_plan.o $(OBJ)/standalone_plan.o $(OBJ)/ouster_hip_capi.o $(STANDALONE:%=$(OBJ)/capi_%.o) $(FEATURES:%=$(OBJ)/capi_%.o) $(OBJ)/host_pool.o
HIP_HDRS := $(CSRC)/ouster_hip_dev.h $(CSRC)/decode_plan.h $(CSRC)/decode_tuner.h $(CSRC)/standalone_plan.h $(CSRC)/host_pool.h $(CSRC)/kernels_common.h $(CSRC)/dwf_dev.h $(CSRC)/wide_tile.h $(CSRC)/launch_util.h $(CSRC)/lds_grant.h $(CSRC)/k_image.h $(CSRC)/k_tonemap.h $(CSRC)/tonemap_dev.h $(CSRC)/k_frame_ops.h $(CSRC)/k_pose.h $(CSRC)/pose_host.h $(CSRC)/k_normals.h $(CSRC)/normals_host.h $(CSRC)/k_voxel.h $(CSRC)/voxel_host.h $(CSRC)/voxel_dev.h $(CSRC)/k_voxel_map.h $(CSRC)/voxel_map_host.h $(CSRC)/k_icp.h $(CSRC)/icp_host.h $(CSRC)/icp_sums_dev.h $(CSRC)/voxel_map_dev.h $(CSRC)/capi_voxel_map.h $(CSRC)/k_registration.h $(CSRC)/registration_host.h $(CSRC)/capi_internal.h $(CSRC)/carve.h include/ouster_hip.h
ROCM ?= /opt/rocm
CXXFLAGS := -O2 -std=c++17 -fPIC -pthread -Wall -Wextra -Iinclude -I$(CSRC)/host -I$(ROCM)/include -D__HIP_PLATFORM_AMD__

PYEXT := ouster_sdk_amd/core$(shell python3-config --extension-suffix)
PYINC := $(shell python3 -m pybind11 --includes)

PLAN_TOOL := tools/_build/standalone_plan_tool

all: $(LIB)/libouster_hip.so $(LIB)/libouster_core_amd.so $(PYEXT) oracle cpptests $(PLAN_TOOL)

$(OBJ)/k_decode_stream_%.o: $(CSRC)/k_decode_stream.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DOUSTER_SPEC_ID=$* -c -o $@ $<

$(OBJ)/k_decode_%.o: $(CSRC)/k_decode.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DOUSTER_SPEC_ID=$* -c -o $@ $<

# no FMA contraction in kernels held to models that round every step on its own, none in their plain C++ halves (host/*_util.cpp):
#   k_image      the display images round like the reference's host build
#   k_tonemap    LocalToneMapper and the luminance percentiles equal tests/tonemap_model.py
#   k_frame_ops  compares converted values only; kept so that no later arithmetic can feed a comparison fused
#   k_pose       interp_pose / transform equal tests/pose_model.py
#   k_normals    normals equals tests/normals_model.py
#   k_voxel      the sums are left folds of single IEEE operations (tests/voxel_model.py)
#   k_voxel_map  admission and the nearest-neighbour query equal tests/voxel_map_model.py
#   k_icp        correspondences, residuals, median and the terms of the sums equal tests/icp_model.py
#   k_registration  moved rows, correspondences and the terms of the sums equal tests/registration_model.py
NO_CONTRACT := k_image k_tonemap k_frame_ops k_pose k_normals k_voxel k_voxel_map k_icp k_registration
$(NO_CONTRACT:%=$(OBJ)/%.o): HIPFLAGS += -ffp-contract=off

$(OBJ)/%.o: $(CSRC)/%.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(OBJ)/%_util.o: $(CSRC)/host/%_util.cpp $(CSRC)/%_host.h include/ouster_hip.h
	@mkdir -p $(OBJ)
	$(CXX) -O2 -std=c++17 -fPIC -Wall -Wextra -ffp-contract=off -c -o $@ $<
$(OBJ)/icp_util.o: $(CSRC)/pose_host.h
$(OBJ)/registration_util.o: $(CSRC)/voxel_map_host.h

# the launch plan is plain C++ (tests/cpp builds the same file without HIP)
$(OBJ)/decode_plan.o: $(CSRC)/decode_plan.cpp $(CSRC)/decode_plan.h include/ouster_hip.h
	@mkdir -p $(OBJ)
	$(CXX) -O3 -std=c++17 -fPIC -Wall -Wextra -c -o $@ $<

# so is the launch plan of the standalone kernels
$(OBJ)/standalone_plan.o: $(CSRC)/standalone_plan.cpp $(CSRC)/standalone_plan.h
	@mkdir -p $(OBJ)
	$(CXX) -O3 -std=c++17 -fPIC -Wall -Wextra -c -o $@ $<

# and evaluated on the CPU by a tool of its own: g++ only, no HIP header or library (tests/test_standalone_plan.py)
$(PLAN_TOOL): tools/standalone_plan_tool.cpp $(CSRC)/standalone_plan.cpp $(CSRC)/standalone_plan.h
	@mkdir -p tools/_build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -o $@ tools/standalone_plan_tool.cpp $(CSRC)/standalone_plan.cpp

$(LIB)/libouster_hip.so: $(HIP_OBJS)
	mkdir -p $(LIB)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $(HIP_OBJS)

$(LIB)/libouster_core_amd.so: $(HOST_SRC) $(wildcard include/ouster/core/*.h include/ouster/hip/*.h include/ouster/pcap/*.h include/ouster/osf/*.h include/ouster/algorithm/*.h include/ouster/mapping/*.h) $(CSRC)/host/host_internal.h $(LIB)/libouster_hip.so
	$(CXX) $(CXXFLAGS) -shared -o $@ $(HOST_SRC) -L$(LIB) -louster_hip -L$(ROCM)/lib -lamdhip64 -lz -l:libzstd.so.1 -Wl,-rpath,'$$ORIGIN'

$(PYEXT): $(CSRC)/python/bindings.cpp $(LIB)/libouster_core_amd.so $(wildcard include/ouster/core/*.h include/ouster/algorithm/*.h include/ouster/mapping/*.h)
	$(CXX) -O2 -std=c++17 -fPIC -shared -fvisibility=hidden -Iinclude $(PYINC) -o $@ $(CSRC)/python/bindings.cpp -L$(LIB) -louster_core_amd -louster_hip -Wl,-rpath,'$$ORIGIN/lib'

oracle:
	$(MAKE) -C oracle -s

cpptests: $(LIB)/libouster_core_amd.so
	$(MAKE) -C tests/cpp -s
	$(MAKE) -C tests/cpp -s sanitized   # runs them: the host halves and the header units under ASan / UBSan, programs of their own
	$(MAKE) -C oracle -s refcpptests

clean:
	rm -rf $(LIB) $(OBJ) oracle/_build tests/cpp/_build tools/_build

.PHONY: all oracle clean cpptests
