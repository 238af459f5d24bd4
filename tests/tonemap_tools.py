"""The C++ programs of the tone-map tests (tests/cpp/tonemap_snippet.cpp, tonemap_lanes.cpp, tonemap_ref_main.cpp): built by
tests/cpp/tonemap.mk, which applies the rules and flags of tests/cpp/Makefile to them, and run with the in-tree libraries on the
loader's path.  The counterpart of tests/cpp_tools.py for programs that tests/cpp/Makefile does not list."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(name):
    """make -C tests/cpp -f tonemap.mk _build/<name> -> (path of the executable, environment to run it with)"""
    rocm = os.environ.get("ROCM", "/opt/rocm")
    cpp, lib = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "ouster_sdk_amd", "lib")
    p = subprocess.run(["make", "-C", cpp, "-f", "tonemap.mk", "_build/" + name, "CXX=" + os.environ.get("CXX", "g++"), "ROCM=" + rocm],
                       capture_output=True, text=True)
    assert p.returncode == 0, "make -f tonemap.mk _build/%s failed:\n%s" % (name, (p.stdout + p.stderr)[-3000:])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = lib + ":" + os.path.join(rocm, "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    return os.path.join(cpp, "_build", name), env


def run(name, args, timeout=600):
    """Builds <name> and runs it with args, which must succeed -> the CompletedProcess (stdout and stderr as text)"""
    exe, env = build(name)
    p = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=timeout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p
