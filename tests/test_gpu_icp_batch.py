"""ICP on a resident hip::DeviceFrameBatch, through tests/cpp/icp_batch_tool.cpp: five frames of two sensors filled from the golden
capture OS-1-128_v2.3.0_1024x10_lb_n3.pcap run dewarp, normals, voxel_downsample_with_normals and align_voxels against a moved copy
of the batch's own downloaded voxels (point to plane), then voxel_downsample and align_voxels again (point to point: that call leaves
no voxel normals).  Each result must be bit-identical to ouster_hip_icp_align on those downloads, and within the margin of
tests/icp_model.py: 8 x the difference between the model with left-fold sums and the model with exact sums on these very clouds
(floor 8 * 2^-52 * max(1, |t|)), measured from the model alone.  align_voxels before any voxel call is std::runtime_error."""
import ctypes as C
import os

import numpy as np
import pytest

import cpp_tools
import icp_cases as K
import icp_model as M
from conftest import PCAPS, has_gpu

pytestmark = pytest.mark.gpu

N_FRAMES = 5
VOXEL = 1.5
DIST = 0.5


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("icp_batch")
    res = cpp_tools.run("icp_batch_tool", [os.path.join(PCAPS, "OS-1-128_v2.3.0_1024x10_lb_n3.pcap"), os.path.join(PCAPS, "OS-1-128_v2.3.0_1024x10.json"),
                                           N_FRAMES, VOXEL, DIST, tmp / "o"], timeout=300)
    out = {"stdout": res.stdout}
    for route in ("plane", "point"):
        b = {}
        for name in ("src", "tgt", "tgtn") + (("srcn",) if route == "plane" else ()):
            b[name] = np.fromfile(tmp / ("o.%s.%s" % (route, name)), np.float64).reshape(-1, 3)
        b["pose"] = np.fromfile(tmp / ("o.%s.pose" % route), np.float64)
        out[route] = b
    return out


def test_error_before_any_voxel_call_and_the_route_taken(run):
    assert "pre_voxel_throws 1" in run["stdout"] and "routes 1" in run["stdout"], run["stdout"]
    assert run["plane"]["pose"][19] == 1.0 and run["point"]["pose"][19] == 0.0
    for route in ("plane", "point"):
        assert 1000 < len(run[route]["src"]) < 20000 and len(run[route]["tgt"]) == len(run[route]["src"])


@pytest.mark.parametrize("route", ["plane", "point"])
def test_align_voxels_equals_the_c_abi_and_the_model(run, route):
    import torch
    from ouster_sdk_amd import _capi as capi
    b = run[route]
    plane = route == "plane"
    normals = (b["srcn"], b["tgtn"]) if plane else (None, None)
    pose, stats = b["pose"][:16].reshape(4, 4), b["pose"][16:19]
    # bit-identical to ouster_hip_icp_align on the downloads
    ctx = capi.Context(0)
    try:
        tensors = []

        def ptr(a):
            tensors.append(torch.from_numpy(np.array(a)).cuda())
            return tensors[-1].data_ptr()

        d, keep = K.make_desc(capi, b["src"], b["tgt"], normals[0], normals[1], None, DIST, 20.0, ptr=ptr)
        assert capi.load_hip().ouster_hip_icp_align(ctx.h, C.byref(d)) == capi.OK
        assert K.desc_pose(d).tobytes() == pose.tobytes()
        assert (d.iterations, d.correspondences, d.solved) == tuple(int(v) for v in stats)
    finally:
        ctx.close()
    # within the margin of the model, measured from the model alone on these clouds
    method = M.PLANE if plane else M.POINT
    left_trace, exact_trace = [], []
    left = M.align(method, b["src"], b["tgt"], normals[0], normals[1], None, DIST, 20.0, exact=False, trace=left_trace)
    exact = M.align(method, b["src"], b["tgt"], normals[0], normals[1], None, DIST, 20.0, exact=True, trace=exact_trace)
    assert left[1] == exact[1] and all(np.array_equal(x["nn"], y["nn"]) for x, y in zip(left_trace, exact_trace))
    margin = K.pose_margin(float(np.abs(left[0] - exact[0]).max()), exact[0][:3, 3])
    print("%s: |gpu - exact model| = %.3e, margin %.3e, %d passes, %d correspondences" %
          (route, np.abs(pose - exact[0]).max(), margin, exact[1], exact[2]))
    assert tuple(int(v) for v in stats) == (exact[1], exact[2], 1)
    assert np.abs(pose - exact[0]).max() <= margin
    assert exact[2] > len(b["src"]) // 2 and abs(pose[0, 3] - 0.04) < 0.02       # it found the move
