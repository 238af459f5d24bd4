"""CPU-only: the dynamic-LDS grant (ouster_sdk_amd/csrc/lds_grant.h) that every launcher with more than 48 KB of dynamic LDS
goes through (launch_with_lds, csrc/launch_util.h).

tests/cpp/test_lds_grant.cpp -- g++ only, no HIP header or library -- replaces the runtime by a counter and checks that nothing is
asked at or below 48 KB, that the first request above it asks and an equal or smaller one after it does not, that a larger one
asks again, that devices 0 and 1 are independent, and that devices 16 and -1 are never remembered and never read device 0's
slot.  tests/cpp/Makefile also builds it with the address and undefined-behaviour sanitizers (_build/test_lds_grant_san, a
stand-alone program); both builds are run here."""
import subprocess

import pytest

import cpp_tools


def _tool(name):
    """tests/cpp/_build/<name>, by the rule of tests/cpp/Makefile (g++ only): build() makes it, and this brings it up to date"""
    return cpp_tools.build(name)[0]


@pytest.mark.parametrize("name", ["test_lds_grant", "test_lds_grant_san"])
def test_lds_grant(name):
    r = subprocess.run([_tool(name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lds_grant: ok" in r.stdout, r.stdout + r.stderr


def test_lds_grant_test_links_no_hip_library():
    out = subprocess.run(["ldd", _tool("test_lds_grant")], capture_output=True, text=True).stdout.lower()
    assert "libc" in out and "hip" not in out and "hsa" not in out, out
