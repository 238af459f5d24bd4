"""IcpTarget on the GPU (csrc/k_icp.hip through ouster_hip_icp_target_create / _align / _step, their _host forms and the Python face).
The yardstick is the single-call route, whose own tests (tests/test_gpu_icp.py) hold it to tests/icp_model.py.

A pass (ouster_hip_icp_target_step), two groups of sources in one call each (tests/icp_target_cases.py): per source the neighbour
index and residual of every row, the count, the median and the Huber delta equal K.tie_model bit for bit, with guard elements behind
every per-row output; every sum agrees with math.fsum of the model's terms to the bound tests/test_gpu_icp.py applies to
ouster_hip_icp_step -- (ceil(N / chunk) + 40) * 2^-53 * sum |t|, N the rows of that source -- and equals ouster_hip_icp_step's own
sum bit for bit.  A call has one max_normal_angle_deg, and the 20-row tie case is built for a wide-open gate: on the plane route group
A runs once per gate, so that every source meets K.tie_model itself in a call with all the others (T.tie_model_at).

Whole calls (ouster_hip_icp_target_align): seven sources of 600, 1024, 1025, 1233, 2049, 19 and 20 rows against the realistic target in
one call, which by the model take 2, 3, 4, 8, 7, 0, 2 passes point to point and 2, 3, 3, 4, 1, 0, 2 point to plane
(tests/test_icp_target_api_cpu.py asserts those preconditions).  Pose, iterations, solved and correspondences of every source must
equal, bit for bit, ouster_hip_icp_align on that source alone -- in the given order, in reverse order, and with K = 1 for each."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import icp_cases as K
import icp_model as M
import icp_target_cases as T
from conftest import ROOT, has_gpu
from test_gpu_icp import TREE_LEVELS        # the bound of the sums is that of ouster_hip_icp_step: imported, not restated

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))


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


class Uploads:
    """device copies of host arrays, kept alive"""

    def __init__(self, torch):
        self.torch, self.tensors = torch, []

    def __call__(self, arr):
        t = self.torch.from_numpy(np.array(arr)).cuda()      # a copy: the cached arrays are read-only
        self.tensors.append(t)
        return t.data_ptr()


def make_target(gpu, points, normals, dist, form="device"):
    capi, ctx, torch = gpu
    up = Uploads(torch)
    rc, h = T.create(capi, ctx.h, points, normals, dist, ptr=up if form == "device" else None, host=form != "device")
    assert rc == capi.OK and h.value, last_error(capi)
    return h


# ---- one pass ---------------------------------------------------------------------------------------------------------------------
_steps = {}


def target_step(gpu, plane, which, angle):
    """ouster_hip_icp_target_step on a group, once per case -> [(out, nn with guard, r with guard)] per source, twice"""
    key = (plane, which, angle)
    if key in _steps:
        return _steps[key]
    capi, ctx, torch = gpu
    L = capi.load_hip()
    group = T.step_groups(plane)[which]
    h = make_target(gpu, group["tgt"], group["tgt_n"], K.CELL)
    up = Uploads(torch)
    s, keep, dtype = T.make_sources(capi, [a["src"] for a in group["sources"]], [a["src_n"] for a in group["sources"]] if plane else None, ptr=up)
    k = len(group["sizes"])
    poses = (C.c_double * (16 * k))(*np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in group["poses"]]).tolist())
    runs = []
    for _ in range(2):
        outs = (capi.IcpStepOut * k)()
        held = []
        for i, n in enumerate(group["sizes"]):
            nn = torch.full((n + K.GUARD,), K.GUARD_NN, dtype=torch.int32, device="cuda")
            r = torch.full((n + K.GUARD,), K.GUARD_R, dtype=torch.float64, device="cuda")
            outs[i].nn, outs[i].r = nn.data_ptr(), r.data_ptr()
            held.append((nn, r))
        rc = L.ouster_hip_icp_target_step(ctx.h, h, s, k, dtype, angle, poses, outs)
        assert rc == capi.OK, last_error(capi)
        runs.append([(outs[i], held[i][0].cpu().numpy(), held[i][1].cpu().numpy()) for i in range(k)])
    assert T.sources_untouched(s, k)
    L.ouster_hip_icp_target_destroy(h)
    _steps[key] = runs
    return runs


def single_step(gpu, n, plane, variant, angle):
    """ouster_hip_icp_step on the same source alone -> IcpStepOut"""
    capi, ctx, torch = gpu
    a, pose = K.tie_case(n, plane, variant)
    up = Uploads(torch)
    d, keep = K.make_desc(capi, a["src"], a["tgt"], a["src_n"], a["tgt_n"], None, K.CELL, angle, ptr=up)
    p = (C.c_double * 16)(*np.asarray(pose).reshape(-1).tolist())
    out = capi.IcpStepOut()
    assert capi.load_hip().ouster_hip_icp_step(ctx.h, C.byref(d), p, C.byref(out)) == capi.OK, last_error(capi)
    return out


def group_cases(plane):
    return [(which, angle) for which in (0, 1) for angle in T.step_gates(T.step_groups(plane)[which], plane)]


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_step_correspondences_count_and_median_equal_the_model_bit_for_bit(gpu, plane):
    seen = []
    for which, angle in group_cases(plane):
        group = T.step_groups(plane)[which]
        run = target_step(gpu, plane, which, angle)[0]
        for (out, nn, r), n in zip(run, group["sizes"]):
            want = T.tie_model_at(n, plane, group["variant"], angle)
            what = "group %d angle %g n %d" % (which, angle, n)
            assert (nn[n:] == K.GUARD_NN).all() and (r[n:] == K.GUARD_R).all(), what
            assert np.array_equal(nn[:n], want["nn"]), (what, np.flatnonzero(nn[:n] != want["nn"])[:10])
            assert K.same_bits(r[:n], want["r"]), what
            assert out.count == want["count"] and bool(out.solved) == want["solved"] and bool(out.stop) == want["stop"], what
            assert K.same_bits([out.median, out.huber_delta], [want["median"], want["huber_delta"]]), what
            if want is K.tie_model(n, plane, group["variant"]):
                seen.append(want["count"])
    # every source met K.tie_model itself, and the inputs do what they were built for: matched and unmatched rows in all but the first
    assert sorted(seen) == sorted(T.STEP_COUNTS[plane])
    sizes = [n for g in T.step_groups(plane) for n in g["sizes"]]
    assert all(c == 20 if n == 20 else 20 < c < n for c, n in zip(T.STEP_COUNTS[plane], sizes))


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_step_sums_within_the_bound_of_the_tree_and_equal_to_the_single_call(gpu, plane):
    capi = gpu[0]
    chunk = capi.load_hip().ouster_hip_icp_chunk_rows()
    for which, angle in group_cases(plane):
        group = T.step_groups(plane)[which]
        first, second = target_step(gpu, plane, which, angle)
        for (out, nn_gpu, r_gpu), (again, nn2, r2), n in zip(first, second, group["sizes"]):
            want = T.tie_model_at(n, plane, group["variant"], angle)
            nn, r = want["nn"], want["r"]
            what = "group %d angle %g n %d" % (which, angle, n)
            bound_factor = (math.ceil(n / chunk) + TREE_LEVELS) * 2.0 ** -53
            if not want["solved"]:
                assert list(out.sums) == [0.0] * capi.ICP_SUMS, what
                continue
            if plane:
                groups = [(0, M.terms_plane(nn, r, want["x"], want["q"], out.huber_delta))]
            else:
                cx, cq = list(out.centroid_x), list(out.centroid_q)
                groups = [(0, M.terms_point_a(nn, r, want["x"], want["q"], out.huber_delta)),
                          (7, M.terms_point_b(nn, r, want["x"], want["q"], out.huber_delta, cx, cq))]
                assert K.same_bits(cx + cq, [out.sums[1 + k] / out.sums[0] for k in range(3)] + [out.sums[4 + k] / out.sums[0] for k in range(3)])
            for at, terms in groups:
                for k in range(terms.shape[1]):
                    exact, total = math.fsum(terms[:, k]), math.fsum(np.abs(terms[:, k]))
                    err = abs(out.sums[at + k] - exact)
                    assert err <= bound_factor * total, (what, "sum %d" % (at + k), err, bound_factor * total)
            # the same call twice: the same bits, everywhere
            assert bytes(out)[16:] == bytes(again)[16:] and nn2.tobytes() == nn_gpu.tobytes() and r2.tobytes() == r_gpu.tobytes(), what
            got = np.array(list(out.next_pose)).reshape(4, 4)
            assert np.isfinite(got).all() and np.array_equal(got[3], [0.0, 0.0, 0.0, 1.0])
            # and everything behind the two pointers equals ouster_hip_icp_step on this source alone: equal chunks, equal fold order
            alone = single_step(gpu, n, plane, group["variant"], angle)
            assert bytes(out)[16:] == bytes(alone)[16:], what


# ---- whole calls ------------------------------------------------------------------------------------------------------------------
def clouds(method, dtype=np.float64):
    tgt, tgt_n, sources = T.align_sources()
    plane = method == M.PLANE
    return tgt, (tgt_n if plane else None), [p.astype(dtype) for p, _ in sources], ([n.astype(dtype) for _, n in sources] if plane else None)


_singles = {}


def single_align(gpu, method, k, guess=None, dtype=np.float64):
    """ouster_hip_icp_align on source k alone, device arrays -> (pose bytes, iterations, correspondences, solved)"""
    key = (method, k, None if guess is None else np.asarray(guess).tobytes(), np.dtype(dtype).name)
    if key not in _singles:
        capi, ctx, torch = gpu
        tgt, tgt_n, src, src_n = clouds(method)
        up = Uploads(torch)
        # a float32 source is compared with the single call on the widened source: the single call has one dtype for all four arrays
        p = src[k].astype(dtype).astype(np.float64)
        n = src_n[k].astype(dtype).astype(np.float64) if src_n is not None else None
        d, keep = K.make_desc(capi, p, tgt, n, tgt_n, guess, K.REAL_DIST, 20.0, ptr=up)
        assert capi.load_hip().ouster_hip_icp_align(ctx.h, C.byref(d)) == capi.OK, last_error(capi)
        _singles[key] = (K.desc_pose(d).tobytes(), d.iterations, d.correspondences, d.solved)
    return _singles[key]


def target_align(gpu, h, method, order, form="device", guesses=None, dtype=np.float64, angle=20.0):
    """one ouster_hip_icp_target_align[_host] of the sources `order` -> [(pose bytes, iterations, correspondences, solved)]"""
    capi, ctx, torch = gpu
    L = capi.load_hip()
    tgt, tgt_n, src, src_n = clouds(method, dtype)
    pooled = []
    if form == "device":
        ptr = Uploads(torch)
    elif form == "pooled":
        def ptr(arr):
            p = L.ouster_hip_host_alloc(max(arr.nbytes, 4096), 0)
            assert p
            pooled.append(p)
            C.memmove(p, arr.ctypes.data, arr.nbytes)
            return p
    else:
        ptr = None
    s, keep, tag = T.make_sources(capi, [src[k] for k in order], [src_n[k] for k in order] if src_n is not None else None,
                                  [guesses[k] for k in order] if guesses is not None else None, ptr=ptr)
    fn = L.ouster_hip_icp_target_align if form == "device" else L.ouster_hip_icp_target_align_host
    rc = fn(ctx.h, h, s, len(order), tag, angle)
    for p in pooled:
        L.ouster_hip_host_free(p)
    assert rc == capi.OK, last_error(capi)
    return [(T.source_result(s[i])[0].tobytes(),) + T.source_result(s[i])[1:] for i in range(len(order))]


@pytest.fixture(scope="module")
def targets(gpu):
    capi = gpu[0]
    made = {}
    for method in (M.POINT, M.PLANE):
        tgt, tgt_n, _, _ = clouds(method)
        made[method] = make_target(gpu, tgt, tgt_n, K.REAL_DIST)
    yield made
    for h in made.values():
        capi.load_hip().ouster_hip_icp_target_destroy(h)


@pytest.mark.parametrize("method", [M.POINT, M.PLANE], ids=["point", "plane"])
def test_seven_sources_in_one_call_equal_the_single_call_bit_for_bit(gpu, targets, method):
    capi = gpu[0]
    h = targets[method]
    info = capi.IcpTargetInfo()
    assert capi.load_hip().ouster_hip_icp_target_info_read(h, C.byref(info)) == capi.OK
    tgt = clouds(method)[0]
    assert (info.rows, info.rows_used, info.has_normals, info.max_corr_dist) == (len(tgt), len(tgt), int(method == M.PLANE), K.REAL_DIST)
    assert 0 < info.cells <= len(tgt) and info.device_bytes >= len(tgt) * (3 if method == M.POINT else 6) * 8
    want = [single_align(gpu, method, k) for k in range(7)]
    # the single call walks the path the model walks (its own tests hold its poses to the model's)
    assert [w[1] for w in want] == T.ALIGN_PASSES[method]
    assert [(w[1], w[2], w[3]) for w in want] == [(m[1], m[2], int(m[3])) for m in T.align_model(method)]
    order = list(range(7))
    got = target_align(gpu, h, method, order)
    for k in order:
        assert got[k] == want[k], ("source %d" % k, got[k][1:], want[k][1:])
    back = target_align(gpu, h, method, order[::-1])
    for i, k in enumerate(order[::-1]):
        assert back[i] == want[k], ("reverse order, source %d" % k, back[i][1:], want[k][1:])
    for k in order:
        assert target_align(gpu, h, method, [k]) == [want[k]], "K = 1, source %d" % k


@pytest.mark.parametrize("method", [M.POINT, M.PLANE], ids=["point", "plane"])
def test_host_forms_guesses_and_flat_allocation_counts(gpu, targets, method):
    capi = gpu[0]
    h = targets[method]
    want = [single_align(gpu, method, k) for k in range(7)]
    order = [4, 0, 6, 5, 2]
    for form in ("host", "pooled"):
        got = target_align(gpu, h, method, order, form)
        assert got == [want[k] for k in order], form
    # a guess of its own per source
    guesses = [None, np.array(K.POSE_B), None, None, None, np.array(K.POSE_B), None]
    got = target_align(gpu, h, method, [1, 5, 0], guesses=guesses)
    assert got[0] == single_align(gpu, method, 1, guesses[1]) and got[2] == want[0]
    assert got[1] == (np.array(K.POSE_B).tobytes(), 0, 0, 0)                 # 19 rows: its guess
    # repeated calls of sizes already seen allocate nothing, on the device or pinned
    target_align(gpu, h, method, list(range(7)), "host")
    before = capi.alloc_stats()
    for _ in range(20):
        assert target_align(gpu, h, method, list(range(7)), "host") == want
    after = capi.alloc_stats()
    assert (after["device_allocs"], after["pinned_allocs"]) == (before["device_allocs"], before["pinned_allocs"])


@pytest.mark.parametrize("method", [M.POINT, M.PLANE], ids=["point", "plane"])
def test_float32_sources_against_the_float64_target(gpu, targets, method):
    order = [0, 2, 3]
    got = target_align(gpu, targets[method], method, order, dtype=np.float32)
    for i, k in enumerate(order):
        assert got[i] == single_align(gpu, method, k, dtype=np.float32), k
    assert got[0] != single_align(gpu, method, 0)                              # and the rounding of the source is felt


def test_the_handle_does_not_live_in_the_workspace(gpu, targets):
    """two calls on one handle with a single call of another size between them on the same context; create, destroy, create"""
    capi, ctx, torch = gpu
    L = capi.load_hip()
    first = target_align(gpu, targets[M.POINT], M.POINT, [1, 3])
    src, tgt, _ = K.published_point()
    up = Uploads(torch)
    d, keep = K.make_desc(capi, src, tgt, max_corr_dist=0.5, ptr=up)
    assert L.ouster_hip_icp_align(ctx.h, C.byref(d)) == capi.OK
    _singles.clear()
    big = single_align(gpu, M.PLANE, 4)           # and one that lays the workspace out over more rows
    assert target_align(gpu, targets[M.POINT], M.POINT, [1, 3]) == first == [single_align(gpu, M.POINT, 1), single_align(gpu, M.POINT, 3)]
    assert target_align(gpu, targets[M.PLANE], M.PLANE, [4]) == [big]
    tgt_r = clouds(M.POINT)[0]
    frees = capi.alloc_stats()["device_frees"]
    h = make_target(gpu, tgt_r, None, K.REAL_DIST)
    one = target_align(gpu, h, M.POINT, [2])
    L.ouster_hip_icp_target_destroy(h)
    assert capi.alloc_stats()["device_frees"] == frees + 1
    h = make_target(gpu, tgt_r, None, K.REAL_DIST, form="host")
    assert target_align(gpu, h, M.POINT, [2]) == one == [single_align(gpu, M.POINT, 2)]
    # a target made by another context is refused, outputs untouched
    other = capi.Context(0)
    try:
        s, keep, tag = T.make_sources(capi, [clouds(M.POINT)[2][0]], ptr=Uploads(torch))
        assert L.ouster_hip_icp_target_align(other.h, h, s, 1, tag, 20.0) == capi.ERR_INVALID_ARGUMENT
        assert last_error(capi) == "icp_target: made by another context" and T.sources_untouched(s, 1)
    finally:
        other.close()
    L.ouster_hip_icp_target_destroy(h)


def test_a_target_outside_the_grid_is_refused_at_create(gpu):
    capi, ctx, torch = gpu
    tgt, tgt_n, _, _ = clouds(M.PLANE)
    far = tgt.copy()
    far[1234, 1] = 1e12
    stats = capi.alloc_stats()
    for normals, message in ((None, M.MSG_GRID[0]), (tgt_n, M.MSG_GRID[1])):
        for host in (False, True):
            rc, h = T.create(capi, ctx.h, far, normals, K.REAL_DIST, ptr=None if host else Uploads(torch), host=host)
            assert rc == capi.ERR_INVALID_ARGUMENT and last_error(capi) == message and h.value is None
    after = capi.alloc_stats()
    assert after["device_allocs"] - stats["device_allocs"] == after["device_frees"] - stats["device_frees"]       # nothing leaked
    # with its normal gone the far row takes no part, and the target is made: one row fewer in it
    bad_n = tgt_n.copy()
    bad_n[1234] = 0.0
    rc, h = T.create(capi, ctx.h, far, bad_n, K.REAL_DIST)
    assert rc == capi.OK, last_error(capi)
    info = capi.IcpTargetInfo()
    assert capi.load_hip().ouster_hip_icp_target_info_read(h, C.byref(info)) == capi.OK and (info.rows, info.rows_used) == (len(far), len(far) - 1)
    capi.load_hip().ouster_hip_icp_target_destroy(h)


@pytest.mark.parametrize("method", [M.POINT, M.PLANE], ids=["point", "plane"])
def test_python_face(gpu, method):
    import ouster.sdk.algorithm as algorithm
    tgt, tgt_n, src, src_n = clouds(method)
    want = [single_align(gpu, method, k) for k in range(7)]
    with algorithm.IcpTarget(tgt, tgt_n, max_corr_dist=K.REAL_DIST) as t:
        assert t.size == len(tgt) and t.has_normals == (method == M.PLANE) and t.device_bytes > 0
        got = t.align_many(src, src_n)
        assert got.shape == (7, 4, 4) and [got[k].tobytes() for k in range(7)] == [w[0] for w in want]
        one = t.align(src[3], src_n[3] if src_n is not None else None)
        assert one.tobytes() == want[3][0]
        guess = np.array(K.POSE_B)
        assert t.align(src[1], src_n[1] if src_n is not None else None, guess).tobytes() == single_align(gpu, method, 1, guess)[0]
    if method == M.PLANE:
        assert algorithm.point_to_plane_align(src[2], tgt, src_n[2], tgt_n, max_corr_dist=K.REAL_DIST).tobytes() == want[2][0]
    else:
        assert algorithm.point_to_point_align(src[2], tgt, max_corr_dist=K.REAL_DIST).tobytes() == want[2][0]
