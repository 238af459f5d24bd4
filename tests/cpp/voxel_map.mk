# The C++ programs of the voxel map tests, into _build/ like the others (tests/test_voxel_map_api_cpu.py asks for them by name):
#   make -C tests/cpp -f voxel_map.mk [_build/<name>]
# A makefile of its own next to Makefile, which it includes for the variables (CXXFLAGS, LIBS, API_DEPS: one place states the
# flags) and leaves as it is (LANE_DEPS too).
#   voxel_map_batch_tool      a driver of the host API for the GPU tests (TOOLS)
#   voxel_map_snippet         a C++ caller of the public header, -Werror (SNIPPETS)
#   voxel_map_lanes           kernel source compiled for the host, one thread per lane (LANES)
#   voxel_map_ref_sanitized   the plain C++ half of the map (csrc/host/voxel_map_util.cpp) under ASan / UBSan: no GPU, no library.
#                             `make -C tests/cpp -f voxel_map.mk voxel_map_ref_sanitized` builds and runs it.
include Makefile
.DEFAULT_GOAL := voxel_map

VOXEL_MAP := voxel_map_batch_tool voxel_map_snippet voxel_map_lanes voxel_map_ref_sanitized
VOXEL_MAP_HOST := $(CSRC)/host/voxel_map_util.cpp

voxel_map: $(addprefix _build/,$(VOXEL_MAP))

_build/voxel_map_snippet: CXXFLAGS += -Werror
_build/voxel_map_batch_tool _build/voxel_map_snippet: _build/%: %.cpp $(API_DEPS)
	@mkdir -p _build
	$(CXX) $(CXXFLAGS) -o $@ $< $(LIBS)

_build/voxel_map_lanes: voxel_map_lanes.cpp $(LANE_DEPS)
	@mkdir -p _build
	$(CXX) -O1 -std=c++20 -ffp-contract=off -pthread -Ihost_lanes -I. -I$(ROOT)/include -o $@ $(filter %.cpp,$^)

_build/voxel_map_ref_sanitized: voxel_map_ref_main.cpp $(VOXEL_MAP_HOST) $(CSRC)/voxel_map_host.h
	@mkdir -p _build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o $@ voxel_map_ref_main.cpp $(VOXEL_MAP_HOST)
voxel_map_ref_sanitized: _build/voxel_map_ref_sanitized
	_build/voxel_map_ref_sanitized

.PHONY: voxel_map voxel_map_ref_sanitized
