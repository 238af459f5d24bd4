"""The public surface of ICP, checked without a GPU: C ABI symbols and struct layout; the host restatement (ouster_hip_icp_step_ref,
ouster_hip_icp_align_ref) against tests/icp_model.py pass by pass -- neighbour indices, residuals, count, median, Huber delta and the
left-fold sums bit for bit (the weights are a function of the residuals and the delta, and every sum's terms carry them), the pose
after each pass within the solver margin; every error through the C ABI, through Python and through C++ (tests/cpp/icp_snippet.cpp);
and the loud failure of the GPU entry points without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import cpp_tools
import icp_cases as K
import icp_model as M
from conftest import ROOT, has_gpu
from ouster_sdk_amd import _capi as capi

sys.path.insert(0, os.path.join(ROOT, "ouster_sdk_amd", "compat"))

SYMBOLS = ["ouster_hip_icp_align", "ouster_hip_icp_align_host", "ouster_hip_icp_align_ref", "ouster_hip_icp_step",
           "ouster_hip_icp_step_ref", "ouster_hip_icp_timing", "ouster_hip_icp_phase_ms"]
# what a pose after a pass may differ by: the host code follows the model's solver operation for operation (sin and cos come from
# two libraries), so the floor of the solver margin (icp_cases.pose_margin) is all that is granted
POSE_TOL = 8.0 * 2.0 ** -52


def last_error():
    return capi.load_hip().ouster_hip_last_error().decode()


def test_symbols_are_declared_and_exported():
    L = capi.load_hip()
    header = open(os.path.join(ROOT, "include", "ouster_hip.h")).read()
    for name in SYMBOLS:
        assert name in capi.ABI_SYMBOLS and hasattr(L, name) and ("int " + name + "(") in header, name
    assert "uint32_t ouster_hip_icp_chunk_rows(void);" in header and L.ouster_hip_icp_chunk_rows() >= 64
    assert C.sizeof(capi.IcpDesc) == 4 * 8 + 8 * 8 + 2 * 4 + 16 * 8 + 2 * 8 + 16 * 8 + 2 * 4 + 8
    assert C.sizeof(capi.IcpStepOut) == 2 * 8 + 8 + 2 * 8 + (27 + 6 + 16) * 8 + 2 * 4
    assert "#define OUSTER_HIP_ICP_PHASES %d" % len(capi.ICP_PHASES) in header
    assert "#define OUSTER_HIP_ICP_SUMS %d" % capi.ICP_SUMS in header and capi.ICP_SUMS == M.N_SUMS
    ms = (C.c_float * len(capi.ICP_PHASES))()
    assert L.ouster_hip_icp_timing(None, 1) == capi.ERR_INVALID_ARGUMENT and L.ouster_hip_icp_phase_ms(None, ms) == capi.ERR_INVALID_ARGUMENT


def check_pass(out, nn, r, want, n, what):
    assert (nn[n:] == K.GUARD_NN).all() and (r[n:] == K.GUARD_R).all(), what
    assert np.array_equal(nn[:n], want["nn"]), what
    assert K.same_bits(r[:n], want["r"]), what
    assert out.count == want["count"] and bool(out.solved) == want["solved"] and bool(out.stop) == want["stop"], what
    assert K.same_bits([out.median, out.huber_delta], [want["median"], want["huber_delta"]]), what
    assert K.same_bits(list(out.sums), want["sums"]), what
    assert K.same_bits(list(out.centroid_x) + list(out.centroid_q), list(want["centroid_x"]) + list(want["centroid_q"])), what
    got, exp = np.array(list(out.next_pose)).reshape(4, 4), np.array(want["next_pose"])
    assert np.abs(got - exp).max() <= POSE_TOL * max(1.0, np.abs(exp[:3, 3]).max()), (what, got - exp)


@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("n,variant", [(20, 0), (65, 0), (257, 1), (1041, 0), (1041, 1)])
def test_step_ref_equals_the_model_on_the_tie_cases(n, plane, variant):
    a, pose = K.tie_case(n, plane, variant)
    d, keep = K.make_desc(capi, a["src"], a["tgt"], a["src_n"], a["tgt_n"], None, K.CELL, K.tie_gate(n))
    rc, out, nn, r = K.step_ref(capi, d, pose)
    assert rc == capi.OK, last_error()
    want = K.tie_model(n, plane, variant)
    assert want["count"] == 20 if n == 20 else 20 < want["count"] < n
    check_pass(out, nn, r, want, n, "n %d plane %d variant %d" % (n, plane, variant))
    assert K.desc_untouched(d)


@pytest.mark.parametrize("method", [M.POINT, M.PLANE])
def test_ref_equals_the_model_pass_by_pass_on_the_realistic_pair(method):
    src, src_n, tgt, tgt_n, _ = K.realistic_pair(1)
    normals = (src_n, tgt_n) if method == M.PLANE else (None, None)
    trace = []
    pose, iterations, count, solved = M.align(method, src, tgt, normals[0], normals[1], None, K.REAL_DIST, 20.0, trace=trace)
    d, keep = K.make_desc(capi, src, tgt, normals[0], normals[1], None, K.REAL_DIST, 20.0)
    for k, want in enumerate(trace):
        at = np.eye(4) if k == 0 else np.array(trace[k - 1]["next_pose"])    # every pass from the model's pose: differences do not pile up
        rc, out, nn, r = K.step_ref(capi, d, at)
        assert rc == capi.OK, last_error()
        check_pass(out, nn, r, want, len(src), "pass %d" % k)
    assert capi.load_hip().ouster_hip_icp_align_ref(C.byref(d)) == capi.OK, last_error()
    assert (d.iterations, d.correspondences, d.solved) == (iterations, count, int(solved))
    assert np.abs(K.desc_pose(d) - pose).max() <= K.pose_margin(0.0, pose[:3, 3]) * len(trace)


def test_ref_on_the_published_cases_and_the_early_returns():
    L = capi.load_hip()
    src, tgt, shift = K.published_point()
    d, keep = K.make_desc(capi, src, tgt, max_corr_dist=0.5)
    assert L.ouster_hip_icp_align_ref(C.byref(d)) == capi.OK, last_error()
    pose = K.desc_pose(d)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], shift, atol=1e-10)
    assert (d.iterations, d.correspondences, d.solved) == M.align(M.POINT, src, tgt, max_corr_dist=0.5)[1:3] + (1,)
    p, t, pn, tn = K.published_plane()
    d, keep = K.make_desc(capi, p.astype(np.float32), t.astype(np.float32), pn.astype(np.float32), tn.astype(np.float32), max_corr_dist=0.5)
    assert L.ouster_hip_icp_align_ref(C.byref(d)) == capi.OK, last_error()
    pose = K.desc_pose(d)
    np.testing.assert_allclose(pose[:3, :3], np.eye(3), atol=1e-10)
    np.testing.assert_allclose(pose[:3, 3], [0.0, 0.0, np.float64(np.float32(0.2))], atol=1e-9)
    guess = np.array(K.POSE_B)
    for a, b in ((src[:19], tgt), (src, tgt[:19])):
        for fn, args in ((L.ouster_hip_icp_align_ref, ()), (L.ouster_hip_icp_align, (None,)), (L.ouster_hip_icp_align_host, (None,))):
            d, keep = K.make_desc(capi, a, b, guess=guess, max_corr_dist=0.5)      # the two GPU forms: no context, nothing launched
            assert fn(*args, C.byref(d)) == capi.OK, last_error()
            assert np.array_equal(K.desc_pose(d), guess) and (d.iterations, d.correspondences, d.solved) == (0, 0, 0)
    far = tgt.copy()
    far[8:] += 100.0
    d, keep = K.make_desc(capi, src, far, guess=guess, max_corr_dist=0.5)
    assert L.ouster_hip_icp_align_ref(C.byref(d)) == capi.OK
    want = M.align(M.POINT, src, far, None, None, guess, 0.5)
    assert np.array_equal(K.desc_pose(d), guess) and (d.iterations, d.correspondences, d.solved) == (want[1], want[2], 0)


def error_cases():
    src, tgt, _ = K.published_point()
    n = np.tile([0.0, 0.0, 1.0], (27, 1))
    nan, inf = float("nan"), float("inf")
    out = tgt.copy()
    out[3, 1] = 3e9
    cases = [(M.MSG_DIST, dict(max_corr_dist=bad)) for bad in (0.0, -1.0, nan, inf)]
    cases += [(M.MSG_DIST, dict(src_n=n[:5], tgt_n=n, max_corr_dist=0.0, max_normal_angle_deg=-1.0))]
    cases += [(M.MSG_ANGLE, dict(src_n=n[:5], tgt_n=n, max_normal_angle_deg=bad)) for bad in (-0.5, 180.5, nan, inf)]
    cases += [(M.MSG_SRC_ROWS, dict(src_n=n[:5], tgt_n=n[:6])), (M.MSG_TGT_ROWS, dict(src_n=n, tgt_n=n[:6]))]
    return src, tgt, n, out, cases


def test_c_abi_validation_comes_before_the_gpu():
    """ctx is NULL in the GPU forms: a validation error must win over it, which shows that nothing touched the GPU."""
    L = capi.load_hip()
    src, tgt, n, out, cases = error_cases()
    cases = cases + [(M.MSG_ONE_SIDE, dict(src_n=n)), (M.MSG_ONE_SIDE, dict(tgt_n=n))]
    eye = (C.c_double * 16)(*np.eye(4).reshape(-1).tolist())
    for message, kw in cases:
        for fn, args in ((L.ouster_hip_icp_align_ref, ()), (L.ouster_hip_icp_align, (None,)), (L.ouster_hip_icp_align_host, (None,))):
            d, keep = K.make_desc(capi, src, tgt, **kw)
            assert fn(*args, C.byref(d)) == capi.ERR_INVALID_ARGUMENT and last_error() == message, (message, last_error())
            assert K.desc_untouched(d)
        d, keep = K.make_desc(capi, src, tgt, **kw)
        step = capi.IcpStepOut()
        assert L.ouster_hip_icp_step(None, C.byref(d), eye, C.byref(step)) == capi.ERR_INVALID_ARGUMENT and last_error() == message
        assert K.step_ref(capi, d, np.eye(4))[0] == capi.ERR_INVALID_ARGUMENT and last_error() == message
    # the out-of-grid target is found by the host code while it builds the grid; the outputs stay untouched
    for normals, message in (((None, None), M.MSG_GRID[0]), ((n, n), M.MSG_GRID[1])):
        d, keep = K.make_desc(capi, src, out, normals[0], normals[1])
        assert L.ouster_hip_icp_align_ref(C.byref(d)) == capi.ERR_INVALID_ARGUMENT and last_error() == message
        assert K.desc_untouched(d)
        rc, _, nn, r = K.step_ref(capi, d, np.eye(4))
        assert rc == capi.ERR_INVALID_ARGUMENT and (nn == K.GUARD_NN).all() and (r == K.GUARD_R).all()


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_gpu_entry_points_without_a_gpu_fail_loudly():
    L = capi.load_hip()
    src, tgt, _ = K.published_point()
    for fn in (L.ouster_hip_icp_align, L.ouster_hip_icp_align_host):
        d, keep = K.make_desc(capi, src, tgt, max_corr_dist=0.5)
        assert fn(None, C.byref(d)) == capi.ERR_INVALID_ARGUMENT and last_error() == "ctx is NULL" and K.desc_untouched(d)
    from ouster_sdk_amd import core as amd
    with pytest.raises(RuntimeError):
        amd.point_to_point_align(src, tgt, max_corr_dist=0.5)


def test_python_face_names_defaults_and_errors():
    import ouster.sdk.algorithm as algorithm
    from ouster_sdk_amd import core as amd
    assert algorithm.point_to_point_align is amd.point_to_point_align and algorithm.point_to_plane_align is amd.point_to_plane_align
    src, tgt, n, out, cases = error_cases()
    for message, kw in cases:
        with pytest.raises(ValueError) as e:
            if "src_n" in kw:
                amd.point_to_plane_align(src, tgt, kw["src_n"], kw["tgt_n"], None, kw.get("max_corr_dist", 0.25),
                                         kw.get("max_normal_angle_deg", 20.0))
            else:
                amd.point_to_point_align(source_points=src, target_points=tgt, initial_guess=None, **kw)
        assert str(e.value) == message
    with pytest.raises(ValueError, match="source_points must be Nx3"):
        amd.point_to_point_align(np.zeros((30, 4)), tgt)
    with pytest.raises(ValueError, match="initial_guess must be 4x4"):
        amd.point_to_point_align(src, tgt, np.eye(3))
    # fewer than 20 rows: the guess, with every keyword of the reference, on any machine
    guess = np.array(K.POSE_B)
    got = amd.point_to_plane_align(source_points=src[:19], target_points=tgt, source_normals=n[:19], target_normals=n,
                                   initial_guess=guess, max_corr_dist=0.5, max_normal_angle_deg=30.0)
    assert got.shape == (4, 4) and got.dtype == np.float64 and np.array_equal(got, guess)
    assert np.array_equal(amd.point_to_point_align(src, tgt[:3]), np.eye(4))


def test_cpp_caller_compiles_links_and_runs():
    """tests/cpp/icp_snippet.cpp, built by tests/cpp/Makefile with the flags of the other C++ tests and -Werror"""
    p = cpp_tools.run("icp_snippet", [], timeout=300)
    assert "validation ok" in p.stdout and "small clouds ok" in p.stdout, p.stdout
    assert p.stdout.splitlines()[-1].startswith("ok" if has_gpu() else "no-gpu"), p.stdout
