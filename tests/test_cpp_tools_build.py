"""CPU-only: every batch tool, snippet and lanes program of tests/cpp builds through tests/cpp_tools.py, i.e. by the rules of
tests/cpp/Makefile and over tests/cpp/batch_fixture.h.  Compiles and links only (the library must be built, as for the snippet
tests); nothing is run, so that a broken fixture header or build rule shows on a machine without a GPU."""
import os

import cpp_tools

BATCH_TOOLS = ["image_batch_tool", "frame_ops_batch_tool", "pose_batch_tool", "normals_batch_tool", "voxel_batch_tool", "icp_batch_tool"]
SNIPPETS = ["image_processing_snippet", "frame_ops_snippet", "pose_snippet", "normals_snippet", "voxel_snippet", "icp_snippet", "tonemap_snippet",
            "tonemap_eigen_snippet"]
LANES = ["normals_lanes", "voxel_lanes", "icp_lanes", "tonemap_lanes"]


def test_every_program_builds():
    for name in BATCH_TOOLS + SNIPPETS + LANES:
        exe, env = cpp_tools.build(name)
        assert os.path.isfile(exe) and os.access(exe, os.X_OK), name
        assert env["LD_LIBRARY_PATH"].startswith(os.path.join(cpp_tools.ROOT, "ouster_sdk_amd", "lib"))
