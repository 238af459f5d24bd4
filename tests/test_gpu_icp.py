"""ICP on the GPU (csrc/k_icp.hip through ouster_hip_icp_step / ouster_hip_icp_align / _host and the Python face) against
tests/icp_model.py.

A pass (ouster_hip_icp_step): the neighbour index and residual of every row, the count and the median equal the model bit for bit,
on inputs built so that the tie rules decide (tests/icp_cases.py) and with guard elements behind both outputs.  Every sum agrees
with math.fsum of the model's terms -- formed from the pass's own huber_delta and centroids -- to (ceil(N / chunk) + 40) * 2^-53 *
sum |t|: the partials are folded serially, and below them the tree is 3 (thread) + 6 (wave) + 3 (LDS) additions deep.  Two calls
give identical bits.

Whole calls: the reference's two published cases within its own tolerances, through the C ABI, the _host form on pooled and on
foreign memory and Python (C++: tests/cpp/icp_snippet.cpp, run by test_icp_api_cpu.py); and the realistic pair of icp_cases.py.
Its tolerance was measured on the CPU from the model alone, as the largest difference over the noise seeds 1 - 5 between the model
with left-fold sums and the model with exact sums:
    point to point 1.4210854715202004e-14 (3 passes, 3482 correspondences in each)
    point to plane 8.187894806610529e-16  (2 passes, 3482 correspondences in each)
The GPU pose must lie within 8 x that of the exact-sum model (floor 8 * 2^-52 * max(1, |t|)).  Seed 1 is the one tested; the test
first asserts that for it both model runs take the same number of passes and pick identical correspondences in every pass."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

import icp_cases as K
import icp_model as M
from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

MEASURED = {M.POINT: 1.4210854715202004e-14, M.PLANE: 8.187894806610529e-16}   # seeds 1 - 5, see above
SEED = 1
TREE_LEVELS = 40


@pytest.fixture(scope="module")
def gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    assert has_gpu()
    ctx = capi.Context(0)
    yield capi, ctx, torch
    ctx.close()


def last_error(capi):
    return capi.load_hip().ouster_hip_last_error().decode()


def sizes(capi):
    chunk = capi.load_hip().ouster_hip_icp_chunk_rows()
    return [20, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 3 * chunk + 17]


_steps = {}


def device_step(gpu, n, plane, variant):
    """ouster_hip_icp_step on tie_case, once per case: (out, nn with guard, r with guard, the same again from a second call)"""
    key = (n, plane, variant)
    if key in _steps:
        return _steps[key]
    capi, ctx, torch = gpu
    a, pose = K.tie_case(n, plane, variant)
    tensors = []

    def ptr(arr):
        t = torch.from_numpy(np.array(arr)).cuda()      # a copy: the cached arrays are read-only
        tensors.append(t)
        return t.data_ptr()

    d, keep = K.make_desc(capi, a["src"], a["tgt"], a["src_n"], a["tgt_n"], None, K.CELL, K.tie_gate(n), ptr=ptr)
    p = (C.c_double * 16)(*np.asarray(pose).reshape(-1).tolist())
    runs = []
    for _ in range(2):
        nn = torch.full((n + K.GUARD,), K.GUARD_NN, dtype=torch.int32, device="cuda")
        r = torch.full((n + K.GUARD,), K.GUARD_R, dtype=torch.float64, device="cuda")
        out = capi.IcpStepOut()
        out.nn, out.r = nn.data_ptr(), r.data_ptr()
        rc = capi.load_hip().ouster_hip_icp_step(ctx.h, C.byref(d), p, C.byref(out))
        assert rc == capi.OK, last_error(capi)
        runs.append((out, nn.cpu().numpy(), r.cpu().numpy()))
    assert K.desc_untouched(d)
    _steps[key] = runs
    return runs


def cases(capi):
    """every size with the identity pose and dense float64 rows; f32 rows with a stride and a non-identity pose at four of them"""
    s = sizes(capi)
    return [(n, 0) for n in s] + [(n, 1) for n in (s[1], s[6], s[8], s[10])]


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_correspondences_equal_the_model_bit_for_bit(gpu, plane):
    capi = gpu[0]
    for n, variant in cases(capi):
        (out, nn, r), _ = device_step(gpu, n, plane, variant)
        want = K.tie_model(n, plane, variant)
        what = "n %d variant %d" % (n, variant)
        assert (nn[n:] == K.GUARD_NN).all() and (r[n:] == K.GUARD_R).all(), what
        assert np.array_equal(nn[:n], want["nn"]), (what, np.flatnonzero(nn[:n] != want["nn"])[:10])
        assert K.same_bits(r[:n], want["r"]), what
        assert out.count == want["count"] and bool(out.solved) == want["solved"], what
        # the inputs do what they were built for: ties, gated rows and rows without a neighbour are all there
        assert want["count"] == 20 if n == 20 else 20 <= want["count"] < n, what


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_median_and_huber_delta_equal_the_model(gpu, plane):
    capi = gpu[0]
    parities = set()
    for n, variant in cases(capi):
        (out, _, _), _ = device_step(gpu, n, plane, variant)
        want = K.tie_model(n, plane, variant)
        parities.add(want["count"] & 1)
        assert K.same_bits([out.median, out.huber_delta], [want["median"], want["huber_delta"]]), (n, variant)
        assert out.median == M.median_abs(want["r"][want["nn"] >= 0])
    assert parities == {0, 1} and K.tie_model(20, plane, 0)["count"] == 20      # odd and even counts, and exactly 20


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_sums_within_the_bound_of_the_tree(gpu, plane):
    capi = gpu[0]
    chunk = capi.load_hip().ouster_hip_icp_chunk_rows()
    for n, variant in cases(capi):
        (out, nn_gpu, r_gpu), (again, nn2, r2) = device_step(gpu, n, plane, variant)
        want = K.tie_model(n, plane, variant)       # nn, r, x and q equal the GPU's (the test above); the delta and centroids are the GPU's own
        nn, r = want["nn"], want["r"]
        bound_factor = (math.ceil(n / chunk) + TREE_LEVELS) * 2.0 ** -53
        if plane:
            groups = [(0, M.terms_plane(nn, r, want["x"], want["q"], out.huber_delta))]
        else:
            cx, cq = list(out.centroid_x), list(out.centroid_q)
            groups = [(0, M.terms_point_a(nn, r, want["x"], want["q"], out.huber_delta)),
                      (7, M.terms_point_b(nn, r, want["x"], want["q"], out.huber_delta, cx, cq))]
            # the centroids are the divisions of the reported sums
            assert K.same_bits(cx + cq, [out.sums[1 + k] / out.sums[0] for k in range(3)] + [out.sums[4 + k] / out.sums[0] for k in range(3)])
        for at, terms in groups:
            for k in range(terms.shape[1]):
                exact, total = math.fsum(terms[:, k]), math.fsum(np.abs(terms[:, k]))
                err = abs(out.sums[at + k] - exact)
                assert err <= bound_factor * total, ("n %d variant %d sum %d" % (n, variant, at + k), err, bound_factor * total)
        # the same call twice: the same bits, everywhere
        assert bytes(out)[16:] == bytes(again)[16:] and nn2.tobytes() == nn_gpu.tobytes() and r2.tobytes() == r_gpu.tobytes()
        # and the pose after the pass is the host solve of exactly these sums
        got = np.array(list(out.next_pose)).reshape(4, 4)
        assert np.isfinite(got).all() and np.array_equal(got[3], [0.0, 0.0, 0.0, 1.0])


def run_align(gpu, form, src, tgt, src_n, tgt_n, guess, dist, angle=20.0):
    """form: 'device', 'host' (foreign numpy memory) or 'pooled' (the pool's page-locked memory) -> the filled desc"""
    capi, ctx, torch = gpu
    L = capi.load_hip()
    tensors, pooled = [], []
    if form == "device":
        def ptr(arr):
            t = torch.from_numpy(np.array(arr)).cuda()      # a copy: the cached arrays are read-only
            tensors.append(t)
            return t.data_ptr()
    elif form == "pooled":
        def ptr(arr):
            p = L.ouster_hip_host_alloc(max(arr.nbytes, 4096), 0)
            assert p
            pooled.append(p)
            C.memmove(p, arr.ctypes.data, arr.nbytes)
            return p
    else:
        ptr = None
    d, keep = K.make_desc(capi, src, tgt, src_n, tgt_n, guess, dist, angle, ptr=ptr)
    fn = L.ouster_hip_icp_align if form == "device" else L.ouster_hip_icp_align_host
    rc = fn(ctx.h, C.byref(d))
    for p in pooled:
        L.ouster_hip_host_free(p)
    return rc, d


@pytest.mark.parametrize("form", ["device", "host", "pooled"])
def test_published_cases_through_the_c_abi(gpu, form):
    capi = gpu[0]
    src, tgt, shift = K.published_point()
    rc, d = run_align(gpu, form, src, tgt, None, None, None, 0.5)
    assert rc == capi.OK, last_error(capi)
    pose = K.desc_pose(d)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], shift, atol=1e-10)
    assert (d.iterations, d.correspondences, d.solved) == M.align(M.POINT, src, tgt, max_corr_dist=0.5)[1:3] + (1,)
    p, t, pn, tn = K.published_plane()
    rc, d = run_align(gpu, form, p, t, pn, tn, None, 0.5)
    assert rc == capi.OK, last_error(capi)
    pose = K.desc_pose(d)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], [0.0, 0.0, 0.2], atol=1e-9)
    assert (d.iterations, d.correspondences, d.solved) == M.align(M.PLANE, p, t, pn, tn, max_corr_dist=0.5)[1:3] + (1,)


def test_published_cases_through_python(gpu):
    import ouster.sdk.algorithm as algorithm
    src, tgt, shift = K.published_point()
    pose = algorithm.point_to_point_align(src, tgt, max_corr_dist=0.5)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], shift, atol=1e-10)
    p, t, pn, tn = K.published_plane()
    pose = algorithm.point_to_plane_align(p, t, pn, tn, max_corr_dist=0.5)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], [0.0, 0.0, 0.2], atol=1e-9)
    # a guess that is already the answer stays
    guess = np.eye(4)
    guess[:3, 3] = shift
    np.testing.assert_allclose(algorithm.point_to_point_align(src, tgt, guess, 0.5), guess, atol=1e-10)


@functools.lru_cache(maxsize=None)
def realistic_models(method):
    src, src_n, tgt, tgt_n, _ = K.realistic_pair(SEED)
    normals = (src_n, tgt_n) if method == M.PLANE else (None, None)
    left, exact = [], []
    a = M.align(method, src, tgt, normals[0], normals[1], None, K.REAL_DIST, 20.0, exact=False, trace=left)
    b = M.align(method, src, tgt, normals[0], normals[1], None, K.REAL_DIST, 20.0, exact=True, trace=exact)
    return a, b, left, exact


@pytest.mark.parametrize("method", [M.POINT, M.PLANE], ids=["point", "plane"])
def test_realistic_pair_within_the_measured_margin(gpu, method):
    capi = gpu[0]
    a, b, left, exact = realistic_models(method)
    # the precondition of the margin: both model runs walk the same path
    assert a[1] == b[1] and len(left) == len(exact) and all(np.array_equal(x["nn"], y["nn"]) for x, y in zip(left, exact))
    assert np.abs(a[0] - b[0]).max() <= MEASURED[method]
    src, src_n, tgt, tgt_n, move = K.realistic_pair(SEED)
    normals = (src_n, tgt_n) if method == M.PLANE else (None, None)
    margin = K.pose_margin(MEASURED[method], b[0][:3, 3])
    results = []
    for form in ("device", "host"):
        rc, d = run_align(gpu, form, src, tgt, normals[0], normals[1], None, K.REAL_DIST)
        assert rc == capi.OK, last_error(capi)
        pose = K.desc_pose(d)
        print("method %d %s: |gpu - exact model| = %.3e, margin %.3e" % (method, form, np.abs(pose - b[0]).max(), margin))
        assert (d.iterations, d.correspondences, d.solved) == (b[1], b[2], 1)
        assert np.abs(pose - b[0]).max() <= margin
        assert np.abs(pose - move).max() < 5e-3          # and it is the move that was applied
        results.append(pose)
    assert results[0].tobytes() == results[1].tobytes()
    from ouster_sdk_amd import core as amd
    if method == M.PLANE:
        got = amd.point_to_plane_align(src, tgt, src_n, tgt_n, max_corr_dist=K.REAL_DIST)
    else:
        got = amd.point_to_point_align(src, tgt, max_corr_dist=K.REAL_DIST)
    assert got.tobytes() == results[0].tobytes()


def test_timing_reports_the_phases(gpu):
    capi, ctx, _ = gpu
    L = capi.load_hip()
    ms = (C.c_float * len(capi.ICP_PHASES))()
    assert L.ouster_hip_icp_timing(ctx.h, 1) == capi.OK
    assert L.ouster_hip_icp_phase_ms(ctx.h, ms) == capi.ERR_INVALID_ARGUMENT       # no timed call yet
    src, tgt, _ = K.published_point()
    rc, d = run_align(gpu, "device", src, tgt, None, None, None, 0.5)
    assert rc == capi.OK and L.ouster_hip_icp_phase_ms(ctx.h, ms) == capi.OK, last_error(capi)
    assert all(0.0 < v < 1000.0 for v in ms)
    assert L.ouster_hip_icp_timing(ctx.h, 0) == capi.OK


def test_refusals_launch_nothing_and_leave_the_outputs_alone(gpu):
    capi, ctx, torch = gpu
    L = capi.load_hip()
    src, tgt, _ = K.published_point()
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    nan, inf = float("nan"), float("inf")
    cases = [(M.MSG_DIST, dict(max_corr_dist=bad)) for bad in (0.0, -1.0, nan, inf)]
    cases += [(M.MSG_ANGLE, dict(src_n=n, tgt_n=n, max_normal_angle_deg=bad)) for bad in (-0.5, 180.5, nan)]
    cases += [(M.MSG_SRC_ROWS, dict(src_n=n[:5], tgt_n=n)), (M.MSG_TGT_ROWS, dict(src_n=n, tgt_n=n[:6]))]
    cases += [(M.MSG_ONE_SIDE, dict(src_n=n)), (M.MSG_ONE_SIDE, dict(tgt_n=n))]
    stats0 = capi.alloc_stats()
    eye = (C.c_double * 16)(*np.eye(4).reshape(-1).tolist())
    for message, kw in cases:
        # host pointers in the device form: a call that launched anything would fault; it must refuse first
        for fn in (L.ouster_hip_icp_align, L.ouster_hip_icp_align_host):
            d, keep = K.make_desc(capi, src, tgt, **kw)
            assert fn(ctx.h, C.byref(d)) == capi.ERR_INVALID_ARGUMENT and last_error(capi) == message
            assert K.desc_untouched(d)
        d, keep = K.make_desc(capi, src, tgt, **kw)
        nn = np.full(27 + K.GUARD, K.GUARD_NN, np.int32)
        out = capi.IcpStepOut()
        out.nn = nn.ctypes.data
        assert L.ouster_hip_icp_step(ctx.h, C.byref(d), eye, C.byref(out)) == capi.ERR_INVALID_ARGUMENT and last_error(capi) == message
        assert (nn == K.GUARD_NN).all()
    assert capi.alloc_stats()["device_allocs"] == stats0["device_allocs"]
    # the out-of-grid target is found by the kernels: refused with the method's message, outputs behind their guards untouched
    far = tgt.copy()
    far[3, 1] = 3e9
    for normals, message in (((None, None), M.MSG_GRID[0]), ((n, n), M.MSG_GRID[1])):
        for form in ("device", "host"):
            rc, d = run_align(gpu, form, src, far, normals[0], normals[1], None, 0.25)
            assert rc == capi.ERR_INVALID_ARGUMENT and last_error(capi) == message and K.desc_untouched(d)
        tensors = [torch.from_numpy(a).cuda() for a in (src, far, n, n)]
        d, keep = K.make_desc(capi, src, far, normals[0], normals[1], None, 0.25,
                              ptr=lambda a, it=iter(tensors if normals[0] is not None else tensors[:2]): next(it).data_ptr())
        nn = torch.full((27 + K.GUARD,), K.GUARD_NN, dtype=torch.int32, device="cuda")
        r = torch.full((27 + K.GUARD,), K.GUARD_R, dtype=torch.float64, device="cuda")
        out = capi.IcpStepOut()
        out.nn, out.r = nn.data_ptr(), r.data_ptr()
        assert L.ouster_hip_icp_step(ctx.h, C.byref(d), eye, C.byref(out)) == capi.ERR_INVALID_ARGUMENT and last_error(capi) == message
        assert (nn.cpu().numpy() == K.GUARD_NN).all() and (r.cpu().numpy() == K.GUARD_R).all()
    # with its normal gone the far row takes no part, and the call goes through
    bad_n = n.copy()
    bad_n[3] = 0.0
    rc, d = run_align(gpu, "host", src, far, n, bad_n, None, 0.25)
    assert rc == capi.OK, last_error(capi)
    # a second call of a size already seen allocates nothing
    src_r, src_n, tgt_r, tgt_n, _ = K.realistic_pair(SEED)
    run_align(gpu, "host", src_r, tgt_r, src_n, tgt_n, None, K.REAL_DIST)
    before = capi.alloc_stats()["device_allocs"]
    run_align(gpu, "host", src_r, tgt_r, src_n, tgt_n, None, K.REAL_DIST)
    assert capi.alloc_stats()["device_allocs"] == before
