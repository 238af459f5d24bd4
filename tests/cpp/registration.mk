# The C++ programs of the registration tests, into _build/ like the others (tests/test_registration_api_cpu.py asks for the snippet
# by name):
#   make -C tests/cpp -f registration.mk [_build/<name>]
# A makefile of its own next to Makefile, which it includes for the variables (CXXFLAGS, LIBS, API_DEPS: one place states the
# flags) and leaves as it is.
#   registration_batch_tool      a driver of the host API for the GPU tests (TOOLS)
#   registration_lanes           kernel source compiled for the host, one thread per lane (LANES)
#   registration_snippet         a C++ caller of the public headers, -Werror (SNIPPETS)
#   registration_ref_sanitized   the plain C++ half (csrc/host/registration_util.cpp over voxel_map_util.cpp) under ASan / UBSan: no
#                                GPU, no library.  `make -C tests/cpp -f registration.mk registration_ref_sanitized` builds and runs it.
include Makefile
.DEFAULT_GOAL := registration

REGISTRATION := registration_batch_tool registration_snippet registration_lanes registration_ref_sanitized
REGISTRATION_HOST := $(CSRC)/host/registration_util.cpp $(CSRC)/host/voxel_map_util.cpp

registration: $(addprefix _build/,$(REGISTRATION))

_build/registration_snippet: CXXFLAGS += -Werror
_build/registration_batch_tool _build/registration_snippet: _build/%: %.cpp $(API_DEPS)
	@mkdir -p _build
	$(CXX) $(CXXFLAGS) -o $@ $< $(LIBS)

_build/registration_lanes: registration_lanes.cpp $(LANE_DEPS)
	@mkdir -p _build
	$(CXX) -O1 -std=c++20 -ffp-contract=off -pthread -Ihost_lanes -I. -I$(ROOT)/include -o $@ $(filter %.cpp,$^)

_build/registration_ref_sanitized: registration_ref_main.cpp $(REGISTRATION_HOST) $(CSRC)/registration_host.h $(CSRC)/voxel_map_host.h
	@mkdir -p _build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -o $@ registration_ref_main.cpp $(REGISTRATION_HOST)
registration_ref_sanitized: _build/registration_ref_sanitized
	_build/registration_ref_sanitized

.PHONY: registration registration_ref_sanitized
