"""IcpTarget on a resident hip::DeviceFrameBatch, through tests/cpp/icp_target_batch_tool.cpp on the fixture of
tests/test_gpu_icp_batch.py: five frames of two sensors from the golden capture run dewarp, normals and
voxel_downsample_with_normals (then voxel_downsample).  make_icp_target() turns the batch's voxel rows into a resident target, and
align_voxels(target, guess) from a small move must equal the existing pointer overload on the same rows bit for bit -- pose,
iterations, correspondences, solved and the route -- on the point-to-plane and on the point-to-point route, with a call of the
pointer overload between two calls on the handle.  Last the batch is destroyed before its target aligns once more, from host rows:
the target shares the batch's context and outlives it."""
import os

import numpy as np
import pytest

import cpp_tools
import icp_target_cases as T
from conftest import PCAPS, has_gpu

pytestmark = pytest.mark.gpu

N_FRAMES = 5
VOXEL = 1.5
DIST = 0.5


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("icp_target_batch")
    res = cpp_tools.run("icp_target_batch_tool", [os.path.join(PCAPS, "OS-1-128_v2.3.0_1024x10_lb_n3.pcap"),
                                                  os.path.join(PCAPS, "OS-1-128_v2.3.0_1024x10.json"), N_FRAMES, VOXEL, DIST, tmp / "o"], timeout=300)
    out = {"stdout": res.stdout}
    for route in ("plane", "point"):
        out[route] = {name: np.fromfile(tmp / ("o.%s.%s" % (route, name)), np.float64) for name in ("target", "pointer", "info")}
    return out


def test_errors_before_any_voxel_call_and_for_the_wrong_method(run):
    assert "pre_voxel_throws 1" in run["stdout"] and "wrong_method_throws 1" in run["stdout"] and "repeatable 1" in run["stdout"], run["stdout"]
    # the batch is destroyed, then its target aligns once more: the same bits
    assert "outlives_batch 1" in run["stdout"], run["stdout"]


@pytest.mark.parametrize("route", ["plane", "point"])
def test_align_voxels_against_the_target_equals_the_pointer_overload(run, route):
    b = run[route]
    rows, has_normals, device_bytes = b["info"]
    assert 1000 < rows < 20000 and has_normals == (route == "plane") and device_bytes >= rows * (6 if route == "plane" else 3) * 8
    assert b["target"].tobytes() == b["pointer"].tobytes()
    pose, (iterations, correspondences, solved, plane) = b["target"][:16].reshape(4, 4), b["target"][16:]
    assert solved == 1.0 and plane == (route == "plane") and iterations >= 2 and correspondences > rows // 2
    # the batch against its own rows: from the small move back to the identity, to within the loop's stop rule (1e-3 m, 1e-4 rad)
    assert np.abs(pose - np.eye(4)).max() < 1e-3
