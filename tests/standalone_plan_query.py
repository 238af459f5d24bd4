"""Asks tools/_build/standalone_plan_tool (tools/standalone_plan_tool.cpp: g++ only, no HIP library) what ouster_sdk_amd/csrc/standalone_plan.cpp plans for a
standalone launch.  Shared by tests/test_standalone_plan.py and tests/test_gpu_standalone_routes.py."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "_build", "standalone_plan_tool")


def query(lines):
    """One plan (a dict) per query line."""
    assert os.path.exists(TOOL), "tools/_build/standalone_plan_tool is missing: build() makes it"
    lines = list(lines)
    r = subprocess.run([TOOL], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


def destagger_line(row_bytes, aligned=True, rows_env=-1, h=1, n=1):
    return f"destagger row_bytes={row_bytes} aligned={int(aligned)} rows_env={rows_env} h={h} n={n}"


def cartesian_line(w, h, n, vec_ok=True, tile=64):
    return f"cartesian w={w} h={h} n={n} vec_ok={int(vec_ok)} tile={tile}"


def dewarp_line(w, h, n, aligned=True, tile=64):
    return f"dewarp w={w} h={h} n={n} aligned={int(aligned)} tile={tile}"


def destagger(row_bytes, aligned=True, rows_env=-1, h=1, n=1):
    return query([destagger_line(row_bytes, aligned, rows_env, h, n)])[0]


def cartesian(w, h, n, vec_ok=True, tile=64):
    return query([cartesian_line(w, h, n, vec_ok, tile)])[0]


def dewarp(w, h, n, aligned=True, tile=64):
    return query([dewarp_line(w, h, n, aligned, tile)])[0]


def smallest_n_for_group(w, h, group, tile=64, limit=1 << 20):
    """The smallest n_images at which plan_cartesian puts `group` images into one workgroup (binary search over the plan
    function: images_per_block never decreases with n_images)."""
    lo, hi = 1, limit
    assert cartesian(w, h, hi, True, tile)["images_per_block"] >= group
    while lo < hi:
        mid = (lo + hi) // 2
        if cartesian(w, h, mid, True, tile)["images_per_block"] >= group:
            hi = mid
        else:
            lo = mid + 1
    return lo
