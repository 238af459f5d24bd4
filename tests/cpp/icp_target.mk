# The C++ programs of the IcpTarget tests, into _build/ like the others (tests/icp_target_cases.py asks for them by name):
#   make -C tests/cpp -f icp_target.mk [_build/<name>]
# A makefile of its own next to Makefile, which it includes for the variables (CXXFLAGS, LIBS, API_DEPS, LANE_DEPS: one place
# states the flags) and leaves as it is.  One program per class of Makefile, each by that class's recipe:
#   icp_target_batch_tool     a driver of the host API for the GPU tests (TOOLS)
#   icp_target_snippet        a C++ caller of the public header, -Werror (SNIPPETS)
#   icp_target_lanes          kernel source compiled for the host, one thread per lane (LANES), with the plain C++ half of ICP for
#                             its chunk-table builder
#   icp_target_ref_sanitized  the plain C++ helpers of the many-source route under ASan / UBSan: no GPU, no library.
#                             `make -C tests/cpp -f icp_target.mk icp_target_ref_sanitized` builds and runs it.
include Makefile
.DEFAULT_GOAL := icp_target

ICP_TARGET := icp_target_batch_tool icp_target_snippet icp_target_lanes icp_target_ref_sanitized
ICP_HOST := $(CSRC)/host/icp_util.cpp $(CSRC)/host/pose_util.cpp

icp_target: $(addprefix _build/,$(ICP_TARGET))

_build/icp_target_snippet: CXXFLAGS += -Werror
_build/icp_target_batch_tool _build/icp_target_snippet: _build/%: %.cpp $(API_DEPS)
	@mkdir -p _build
	$(CXX) $(CXXFLAGS) -o $@ $< $(LIBS)

_build/icp_target_lanes: icp_target_lanes.cpp $(ICP_HOST) $(LANE_DEPS)
	@mkdir -p _build
	$(CXX) -O1 -std=c++20 -ffp-contract=off -pthread -Ihost_lanes -I. -I$(ROOT)/include -o $@ $(filter %.cpp,$^)

_build/icp_target_ref_sanitized: icp_target_ref_main.cpp $(ICP_HOST) $(CSRC)/icp_host.h $(CSRC)/pose_host.h
	@mkdir -p _build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o $@ icp_target_ref_main.cpp $(ICP_HOST)
icp_target_ref_sanitized: _build/icp_target_ref_sanitized
	_build/icp_target_ref_sanitized

.PHONY: icp_target icp_target_ref_sanitized
