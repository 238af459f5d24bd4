"""interp_pose and transform on the GPU.  interp_pose is held to the long-double truth of tests/golden/pose_vectors.npz within
8 x the reference arithmetic's own error on the case (tests/golden/make_pose_golden.py; bit-exactness is not available: sin / cos
/ acos are not correctly rounded on either side); float results must be float32 of the double result, within one float ulp of
the truth.  transform has exactly one correct bit pattern: the oracle's dense dewarp with the one pose repeated.  Device outputs
lie between guard bytes of 0xCD that must stay."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import pose_model as M
from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))
VECTORS = np.load(os.path.join(ROOT, "tests", "golden", "pose_vectors.npz"))
GUARD = 256
worst_seen = [0.0]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert has_gpu()
    ctx = capi.Context(0)
    yield capi, ctx, torch
    ctx.close()


def case(name, n=None):
    xk, poses, xi = VECTORS[name + "/x_known"], VECTORS[name + "/poses_known"], VECTORS[name + "/x_interp"]
    truth = VECTORS[name + "/truth"]
    if n is not None and n < len(xi):   # evenly spread over the sorted x, both ends kept when there is room for them
        pick = np.unique(np.round(np.linspace(0, len(xi) - 1, n)).astype(int)) if n > 1 else np.array([len(xi) // 2])
        assert len(pick) == n
        xi, truth = xi[pick], truth[pick]
    lim = M.bound(None, VECTORS[name + "/model_err"], VECTORS[name + "/scale"])
    unit = M.EPS * float(VECTORS[name + "/scale"])
    return xk, poses, np.ascontiguousarray(xi), truth, lim, unit


def check_double(got, truth, lim, unit, what):
    got = np.asarray(got).reshape(-1, 16)
    err = float(np.abs(got[:, :12] - truth).max()) if len(got) else 0.0
    worst_seen[0] = max(worst_seen[0], err / unit)
    print("%s: max |got - truth| = %.3g = %.2f eps x scale (allowed %.3g)" % (what, err, err / unit, lim))
    assert err <= lim, what
    assert np.array_equal(got[:, 12:], np.tile([0.0, 0.0, 0.0, 1.0], (len(got), 1))), what


def check_float(got32, got64, truth, what):
    got32, got64 = np.asarray(got32).reshape(-1, 16), np.asarray(got64).reshape(-1, 16)
    assert got32.dtype == np.float32 and np.array_equal(got32, got64.astype(np.float32)), what
    t32 = truth.astype(np.float32)
    assert np.all(np.abs(got32[:, :12].astype(np.float64) - truth) <= np.spacing(np.abs(t32)).astype(np.float64)), what


def device_interp(gpu, xi, xk, poses, dtype):
    """through ouster_hip_interp_pose on device memory between guard bytes -> (N, 16)"""
    capi, ctx, torch = gpu
    n, es = len(xi), 8 if dtype == np.float64 else 4
    d_x = torch.from_numpy(xi).cuda()
    raw = torch.full((GUARD + n * 16 * es + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    capi.check(ctx.L.ouster_hip_interp_pose(ctx.h, d_x.data_ptr(), n, xk.ctypes.data, poses.ctypes.data, len(xk),
                                            capi.F64 if es == 8 else capi.F32, raw.data_ptr() + GUARD))
    ctx.sync()
    host = raw.cpu().numpy()
    assert np.all(host[:GUARD] == 0xCD) and np.all(host[GUARD + n * 16 * es:] == 0xCD)
    return host[GUARD:GUARD + n * 16 * es].view(dtype).reshape(n, 16).copy()


@pytest.mark.parametrize("k", [2, 3, 9])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_interp_pose_device(gpu, n, k):
    xk, poses, xi, truth, lim, unit = case("k%d" % k, n)
    if n == 257:   # the whole case: before the first known time, on every known time, inside every segment, after the last
        seg = [M.segment_index(xk, x) for x in xi]
        assert xi[0] < xk[0] and xi[-1] > xk[-1] and np.all(np.isin(xk, xi)) and set(seg) == set(range(k - 1))
    got = device_interp(gpu, xi, xk, poses, np.float64)
    check_double(got, truth, lim, unit, "k %d n %d" % (k, n))
    got32 = device_interp(gpu, xi, xk, poses, np.float32)
    check_float(got32, got, truth, "float k %d n %d" % (k, n))


@pytest.mark.parametrize("name", ["translation", "tiny"])
def test_interp_pose_small_angle_cases(gpu, name):
    xk, poses, xi, truth, lim, unit = case(name)
    check_double(device_interp(gpu, xi, xk, poses, np.float64), truth, lim, unit, name)


def test_interp_pose_unsorted_x_and_no_x(gpu):
    """device x is evaluated per element: any order gives the same poses; n == 0 touches nothing"""
    capi, ctx, torch = gpu
    xk, poses, xi, truth, lim, unit = case("k9")
    perm = np.random.default_rng(1).permutation(len(xi))
    got = device_interp(gpu, np.ascontiguousarray(xi[perm]), xk, poses, np.float64)
    assert np.array_equal(got, device_interp(gpu, xi, xk, poses, np.float64)[perm])
    capi.check(ctx.L.ouster_hip_interp_pose(ctx.h, None, 0, xk.ctypes.data, poses.ctypes.data, len(xk), capi.F64, None))


@pytest.mark.parametrize("n", [1, 65, 257])
def test_direct_store_form_gives_the_same_bytes(gpu, n):
    """knob "pose_direct": every lane stores its own row instead of the workgroup's rows going through LDS -- the same bits, the
    same guard bytes, for double and float outputs"""
    capi, ctx, torch = gpu
    xk, poses, xi, truth, lim, unit = case("k9", n)
    staged = [device_interp(gpu, xi, xk, poses, dt) for dt in (np.float64, np.float32)]
    ctx.set_knob("pose_direct", 1)
    try:
        direct = [device_interp(gpu, xi, xk, poses, dt) for dt in (np.float64, np.float32)]
    finally:
        ctx.set_knob("pose_direct", 0)
    assert staged[0].tobytes() == direct[0].tobytes() and staged[1].tobytes() == direct[1].tobytes()


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "foreign"])
def test_host_forms_equal_the_device_form(gpu, pooled):
    capi, ctx, torch = gpu
    L = ctx.L
    xk, poses, xi, truth, lim, unit = case("k3")
    n = len(xi)
    want = device_interp(gpu, xi, xk, poses, np.float64)
    want32 = device_interp(gpu, xi, xk, poses, np.float32)
    blocks = []

    def host(nbytes):
        if not pooled:
            return np.full(nbytes, 0xCD, np.uint8)
        p = L.ouster_hip_host_alloc(max(nbytes, 4096), 1)
        assert L.ouster_hip_host_is_pinned(p, nbytes) == 1
        blocks.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(nbytes, 4096),))[:nbytes]
    try:
        x = host(n * 8)
        x.view(np.float64)[:] = xi
        for dtype, tag, ref in ((np.float64, capi.F64, want), (np.float32, capi.F32, want32)):
            out = host(n * 16 * np.dtype(dtype).itemsize)
            capi.check(L.ouster_hip_interp_pose_host(ctx.h, x.ctypes.data, n, xk.ctypes.data, poses.ctypes.data, len(xk), tag,
                                                     out.ctypes.data))
            assert np.array_equal(out.view(dtype).reshape(n, 16), ref)
        # the pair form on the one segment of the two-pose case; backwards in time within the bound as well
        xk2, poses2, xi2, truth2, lim2, unit2 = case("k2")
        out = np.zeros((len(xi2), 16))
        capi.check(L.ouster_hip_interp_pose_pair_host(ctx.h, xi2.ctypes.data, len(xi2), xk2[0], poses2[0].ctypes.data, xk2[1],
                                                      poses2[1].ctypes.data, capi.F64, out.ctypes.data))
        assert np.array_equal(out, device_interp(gpu, xi2, xk2, poses2, np.float64))
        capi.check(L.ouster_hip_interp_pose_pair_host(ctx.h, xi2.ctypes.data, len(xi2), xk2[1], poses2[1].ctypes.data, xk2[0],
                                                      poses2[0].ctypes.data, capi.F64, out.ctypes.data))
        check_double(out, truth2, lim2, unit2, "pair form, t1 < t0")
        backwards = np.array([1.0, 0.5])
        with pytest.raises(ValueError, match="x_interp values must be monotonically increasing"):
            capi.check(L.ouster_hip_interp_pose_host(ctx.h, backwards.ctypes.data, 2, xk.ctypes.data, poses.ctypes.data,
                                                     len(xk), capi.F64, out.ctypes.data))
    finally:
        for p in blocks:
            L.ouster_hip_host_free(p)


def test_python_face(gpu):
    import ouster.sdk.core as core
    xk, poses, xi, truth, lim, unit = case("k9", 65)
    p44 = poses.reshape(-1, 4, 4)
    got = core.interp_pose(xi, xk, p44)
    assert got.shape == (65, 4, 4) and got.dtype == np.float64
    check_double(got, truth, lim, unit, "python (N,)")
    assert np.array_equal(core.interp_pose(xi.reshape(-1, 1), xk.reshape(-1, 1), p44), got)
    assert np.array_equal(core.interp_pose(xi.copy(), xk, np.asfortranarray(p44)), got)
    # interp_pose_float: float poses in, float poses out; the same as the double form on the poses rounded to float
    got32 = core.interp_pose_float(xi, xk, p44.astype(np.float32))
    assert got32.shape == (65, 4, 4) and got32.dtype == np.float32
    assert np.array_equal(got32, core.interp_pose(xi, xk, p44.astype(np.float32).astype(np.float64)).astype(np.float32))
    assert np.abs(got32.reshape(-1, 16)[:, :12] - truth).max() <= 1e-6 * float(VECTORS["k9/scale"])
    assert core.interp_pose(np.zeros(0), xk, p44).shape == (0, 4, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 64, 1000])
def test_transform_equals_the_oracles_dense_dewarp(gpu, oracle, n, dtype):
    import ouster.sdk.core as core
    capi, ctx, torch = gpu
    rng = np.random.default_rng(n)
    pose = VECTORS["k3/poses_known"][1].reshape(4, 4)
    pts = rng.uniform(-120, 120, (n, 3)).astype(dtype)
    want = oracle.dewarp(pts, np.tile(pose, (n, 1, 1)), 1, n)
    assert want.dtype == dtype and not np.array_equal(want, pts)
    assert np.array_equal(M.transform(pts, pose), want)
    es = np.dtype(dtype).itemsize
    d_p = torch.from_numpy(pts).cuda()
    raw = torch.full((GUARD + n * 3 * es + GUARD,), 0xCD, dtype=torch.uint8, device="cuda")
    capi.check(ctx.L.ouster_hip_transform(ctx.h, d_p.data_ptr(), np.ascontiguousarray(pose).ctypes.data, raw.data_ptr() + GUARD,
                                          capi.F64 if es == 8 else capi.F32, n))
    ctx.sync()
    host = raw.cpu().numpy()
    assert np.all(host[:GUARD] == 0xCD) and np.all(host[GUARD + n * 3 * es:] == 0xCD)
    assert host[GUARD:GUARD + n * 3 * es].view(dtype).reshape(n, 3).tobytes() == want.tobytes()
    out = np.empty_like(pts)
    capi.check(ctx.L.ouster_hip_transform_host(ctx.h, pts.ctypes.data, np.ascontiguousarray(pose).ctypes.data, out.ctypes.data,
                                               capi.F64 if es == 8 else capi.F32, n))
    assert out.tobytes() == want.tobytes()
    # the Python face: (N, 3), and (H, W, 3) where N splits
    got = core.transform(pts, pose.astype(dtype))
    assert got.dtype == dtype and got.shape == (n, 3) and got.tobytes() == want.tobytes()
    if n % 8 == 0:
        got3 = core.transform(pts.reshape(8, n // 8, 3), pose.astype(dtype))
        assert got3.shape == (8, n // 8, 3) and got3.tobytes() == want.tobytes()


def test_report_worst_error():
    print("largest GPU error seen: %.2f eps x scale" % worst_seen[0])
