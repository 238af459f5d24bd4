"""CPU-only: the decode's variant tuner (ouster_sdk_amd/csrc/decode_tuner.h), which picks the kernel ouster_hip_decode launches.

tests/cpp/test_tuner.cpp -- g++ only, no HIP header or library -- replaces the clocks by an array of floats and checks the
sequence of a workload's calls (four samples of each candidate, the default while they are in flight, then the verdict with
nothing asked of the clock), what decides the verdict (the fastest warm sample; the cold one only when no warm one landed; ties
to the earlier candidate; no usable sample, no win; nothing usable, 256), the cache file's text and what is refused at load,
the round trip through a file, `retune`, the bound on the table, that every route by which an entry goes destroys its
samples, and that another candidate list under the same key starts over.  tests/cpp/Makefile also builds it with the address
and undefined-behaviour sanitizers (_build/test_tuner_san, a stand-alone program); both builds are run here."""
import subprocess

import pytest

import cpp_tools


def _tool(name):
    """tests/cpp/_build/<name>, by the rule of tests/cpp/Makefile (g++ only): build() makes it, and this brings it up to date"""
    return cpp_tools.build(name)[0]


@pytest.mark.parametrize("name", ["test_tuner", "test_tuner_san"])
def test_tuner(name):
    r = subprocess.run([_tool(name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tuner: ok" in r.stdout, r.stdout + r.stderr


def test_tuner_test_links_no_hip_library():
    out = subprocess.run(["ldd", _tool("test_tuner")], capture_output=True, text=True).stdout.lower()
    assert "libc" in out and "hip" not in out and "hsa" not in out, out
