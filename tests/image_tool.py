"""Builds tests/cpp/image_batch_tool.cpp (the C++ driver of hip::DeviceFrameBatch::render_images) with the flags of
tests/cpp/Makefile; used by tests/test_gpu_image_processing.py and tools/ab/image_bench.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_tool():
    """-> (path of the executable, environment to run it with)"""
    rocm = os.environ.get("ROCM", "/opt/rocm")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe, lib = os.path.join(out, "image_batch_tool"), os.path.join(ROOT, "ouster_sdk_amd", "lib")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "image_batch_tool.cpp"), "-L" + lib, "-louster_core_amd",
                           "-louster_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + lib,
                           "-Wl,-rpath," + os.path.join(rocm, "lib")])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = lib + ":" + os.path.join(rocm, "lib") + ":" + env.get("LD_LIBRARY_PATH", "")
    return exe, env
