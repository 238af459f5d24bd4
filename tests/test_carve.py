"""CPU-only: the workspace carver (ouster_sdk_amd/csrc/carve.h) that lays out the voxel and ICP workspaces.

tests/cpp/test_carve.cpp -- g++ only, no HIP header or library -- measures and assigns mixed layouts (zero-size pieces, pieces
of 1, 255, 256 and 257 bytes, a piece of 2^31 + 1 bytes that is counted and never touched) and checks that every piece is
256-byte aligned, that pieces do not overlap, that the last one ends within the total, and that the measuring and the
assigning pass agree on the total.  tests/cpp/Makefile also builds it with the address and undefined-behaviour sanitizers
(_build/test_carve_san); this wrapper runs the plain build."""
import subprocess

import cpp_tools


def _tool():
    """tests/cpp/_build/test_carve, by the rule of tests/cpp/Makefile (g++ only): build() makes it, and this brings it up to date"""
    return cpp_tools.build("test_carve")[0]


def test_carve_layouts():
    r = subprocess.run([_tool()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "carve: ok" in r.stdout, r.stdout + r.stderr


def test_carve_test_links_no_hip_library():
    out = subprocess.run(["ldd", _tool()], capture_output=True, text=True).stdout.lower()
    assert "libc" in out and "hip" not in out and "hsa" not in out, out
