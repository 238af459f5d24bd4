# The C++ programs of the tone-map tests (tests/tonemap_tools.py asks for them by name), built by the rules and flags of the
# Makefile beside this file -- it stays the one place that states them -- with its program lists replaced by these:
#   make -C tests/cpp -f tonemap.mk [_build/<name>]
# (tests/cpp/Makefile and tests/cpp_tools.py are test files of earlier features and stay as they are.)
override TOOLS :=
override SNIPPETS := tonemap_snippet
override LANES := tonemap_lanes
override BENCHES :=
override CPU_ONLY := tonemap_ref_sanitized tonemap_eigen_snippet

tonemap: _build/tonemap_snippet _build/tonemap_lanes _build/tonemap_ref_sanitized _build/tonemap_eigen_snippet

include Makefile

# the host half of the display images alone (csrc/host/image_processing.cpp; the C ABI calls it makes are stubs of the program) under
# ASan / UBSan: no GPU, no library.  `make -f tonemap.mk tonemap_ref_sanitized` builds and runs it.
_build/tonemap_ref_sanitized: tonemap_ref_main.cpp $(CSRC)/host/image_processing.cpp $(ROOT)/include/ouster/core/image_processing.h $(ROOT)/include/ouster_hip.h
	@mkdir -p _build
	$(CXX) -O1 -g -std=c++17 -Wall -Wextra -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
	    -I$(ROOT)/include -I$(CSRC)/host -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ -o $@ tonemap_ref_main.cpp $(CSRC)/host/image_processing.cpp
tonemap_ref_sanitized: _build/tonemap_ref_sanitized
	_build/tonemap_ref_sanitized

# the Eigen boundary switch for RgbImgRef (Eigen's Tensor module mocked, like Eigen/Core for eigen_switch_on)
_build/tonemap_eigen_snippet: tonemap_eigen_snippet.cpp mock_eigen/Eigen/Core mock_eigen/unsupported/Eigen/CXX11/Tensor $(API_DEPS)
	@mkdir -p _build
	$(CXX) $(CXXFLAGS) -Werror -DOUSTER_HIP_USE_EIGEN -Imock_eigen -o $@ tonemap_eigen_snippet.cpp $(LIBS)

.PHONY: tonemap tonemap_ref_sanitized
