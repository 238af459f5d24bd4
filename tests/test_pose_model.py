"""tests/pose_model.py, the yardstick of interp_pose / transform, pinned without a GPU: on the results the reference's own test
records (tests/golden/interp_pose_reference.json, at its isApprox(..., 1e-4)), on closed forms, on its branches and on every
error it raises."""
import json
import os

import numpy as np
import pytest

import pose_model as M
from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "interp_pose_reference.json")


def rot_z(angle, t=(0.0, 0.0, 0.0)):
    m = np.eye(4)
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = np.cos(angle), -np.sin(angle), np.sin(angle), np.cos(angle)
    m[:3, 3] = t
    return m


def is_approx(a, b, prec):
    """Eigen's isApprox: ||a - b|| <= prec * min(||a||, ||b||), Frobenius"""
    return np.linalg.norm(a - b) <= prec * min(np.linalg.norm(a), np.linalg.norm(b))


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_reference_recorded_poses(dtype):
    g = json.load(open(GOLD))
    got = M.interp_pose(g["x_interp"], g["x_known"], g["poses_known"], dtype).astype(np.float64)
    want = np.array(g["expected"]).reshape(-1, 4, 4)
    assert got.shape == want.shape == (8, 4, 4)
    for i in range(8):
        assert is_approx(got[i], want[i], g["tolerance"]), (i, got[i], want[i])
    # x == x_known[j] is in the recorded set: 101000 gives the first pose back, 102000 and 103000 the rounded inputs
    known = np.array(g["poses_known"]).reshape(-1, 4, 4)
    for i, j in ((2, 0), (4, 1), (6, 2)):
        assert np.abs(got[i] - known[j]).max() < 1e-5


def test_pure_rotation_about_z_is_the_closed_form():
    a, b = rot_z(0.3), rot_z(1.1)
    x = np.array([9.0, 10.0, 10.25, 11.5, 12.0, 13.0])
    got = M.interp_pose(x, [10.0, 12.0], [a, b])
    for xv, g in zip(x, got):
        want = rot_z(0.3 + (xv - 10.0) / 2.0 * 0.8)
        assert np.abs(g - want).max() < 1e-14, xv


def test_pure_translation_has_a_rotation_twist_of_exactly_zero():
    r = rot_z(0.7)[:3, :3]
    a, b = np.eye(4), np.eye(4)
    a[:3, :3] = b[:3, :3] = r
    a[:3, 3], b[:3, 3] = (1.0, -2.0, 3.0), (11.0, 2.0, -5.0)
    table = M.segments_table([100.0, 104.0], [a, b])
    assert np.array_equal(table[0, 17:20], [0.0, 0.0, 0.0])
    got = M.interp_pose([98.0, 100.0, 101.0, 104.0, 106.0], [100.0, 104.0], [a, b])
    for xv, g in zip([98.0, 100.0, 101.0, 104.0, 106.0], got):
        assert np.abs(g[:3, :3] - r).max() < 1e-15
        assert np.abs(g[:3, 3] - (a[:3, 3] + (xv - 100.0) / 4.0 * (b[:3, 3] - a[:3, 3]))).max() < 1e-13


def test_relative_angle_of_1e_9_takes_the_small_angle_branches():
    a, b = rot_z(0.5, (1.0, 2.0, 3.0)), rot_z(0.5 + 1e-9, (1.0, 2.0, 3.0))
    table = M.segments_table([0.0, 1.0], [a, b])
    w = table[0, 17:20]
    assert np.sum(w * w) <= M.EPS                      # the `/ 2` branch of the log
    assert abs(w[2] - 1e-9) < 1e-15 and w[0] == 0.0 and w[1] == 0.0
    got = M.interp_pose([0.0, 0.5, 1.0], [0.0, 1.0], [a, b])
    for xv, g in zip([0.0, 0.5, 1.0], got):
        assert np.abs(g - rot_z(0.5 + xv * 1e-9, (1.0, 2.0, 3.0))).max() < 1e-14


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_known_times_return_the_known_poses(dtype):
    rng = np.random.default_rng(3)
    poses = [rot_z(a, rng.uniform(-10, 10, 3)) for a in (0.1, 0.9, 1.3, 2.0)]
    xk = [5.0, 5.5, 6.25, 7.0]
    got = M.interp_pose(xk, xk, poses, dtype).astype(np.float64)
    for g, p in zip(got, poses):
        assert np.abs(g - p).max() < 1e-13
    assert [M.segment_index(xk, x) for x in (4.0, 5.0, 5.49, 5.5, 6.25, 6.9, 7.0, 8.0)] == [0, 0, 0, 1, 2, 2, 2, 2]


def test_two_pose_form_runs_backwards_in_time():
    a, b = rot_z(0.2, (0.0, 1.0, 0.0)), rot_z(0.8, (3.0, 1.0, -1.0))
    x = [1.0, 2.0, 3.0, 4.0]
    fwd = M.interp_pose_two(x, 1.0, a, 3.0, b)
    bwd = M.interp_pose_two(x, 3.0, b, 1.0, a)
    assert np.abs(fwd - bwd).max() < 1e-13
    assert np.abs(bwd[0] - a).max() < 1e-14 and np.abs(bwd[2] - b).max() < 1e-14


def test_errors_carry_the_reference_messages():
    eye = np.eye(4)
    with pytest.raises(ValueError, match=M.MSG_FEW):
        M.interp_pose([0.0], [1.0], [eye])
    with pytest.raises(ValueError, match=M.MSG_FEW):
        M.interp_pose([0.0], [], [])
    with pytest.raises(ValueError, match=M.MSG_SIZES):
        M.interp_pose([0.0], [1.0, 2.0], [eye])
    with pytest.raises(ValueError, match=M.MSG_KNOWN):
        M.interp_pose([0.0], [1.0, 1.0], [eye, eye])
    with pytest.raises(ValueError, match=M.MSG_KNOWN):
        M.interp_pose([], [1.0, 2.0, 3.0, 2.5], [eye] * 4)      # the last pair, and no x at all: every pair is checked
    with pytest.raises(ValueError, match=M.MSG_DURATION):
        M.interp_pose_two([0.0], 1.0, eye, 1.0 + 1e-17, eye)
    with pytest.raises(ValueError, match="x_interp values must be monotonically increasing: 1.000000 < 2.000000"):
        M.interp_pose([0.0, 2.0, 1.0], [0.0, 5.0], [eye, eye])
    with pytest.raises(ValueError, match=M.MSG_INTERP):
        M.interp_pose([0.0, 3.0, 2.9], [0.0, 1.0, 2.0], [eye] * 3)   # across segments: where the reference does not look
    with pytest.raises(ValueError, match=M.MSG_INTERP):
        M.interp_pose_two([2.0, 1.0], 0.0, eye, 1.0, eye)


def test_transform_is_r_p_plus_t_in_the_points_type():
    rng = np.random.default_rng(5)
    pose = rot_z(0.4, (1.5, -2.5, 0.125))
    for dt in (np.float32, np.float64):
        pts = rng.uniform(-50, 50, (7, 5, 3)).astype(dt)
        got = M.transform(pts, pose)
        assert got.dtype == dt and got.shape == pts.shape
        want = pts.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
        assert np.abs(got - want).max() <= (1e-4 if dt == np.float32 else 1e-12)
        assert np.array_equal(M.transform(pts.reshape(-1, 3), pose), got.reshape(-1, 3))
    assert np.array_equal(M.transform(pts, np.eye(4)), pts)


def test_fixture_is_what_its_maker_promises():
    v = np.load(os.path.join(ROOT, "tests", "golden", "pose_vectors.npz"))
    names = sorted({k.split("/")[0] for k in v.files})
    assert names == ["k2", "k3", "k9", "tiny", "translation"]
    for name in names:
        xk, poses, xi = v[name + "/x_known"], v[name + "/poses_known"], v[name + "/x_interp"]
        assert float(v[name + "/model_err"]) <= 64.0 and float(v[name + "/table_err"]) <= 64.0
        assert np.all(np.diff(xi) >= 0) and xi[0] >= xk[0] - (xk[1] - xk[0]) and xi[-1] <= xk[-1] + (xk[-1] - xk[-2])
        assert np.all(np.isin(xk, xi)) or len(xi) < len(xk) + 4
        got = M.interp_pose(xi, xk, poses).reshape(-1, 16)
        lim = M.bound(None, v[name + "/model_err"], v[name + "/scale"])
        assert np.abs(got[:, :12] - v[name + "/truth"]).max() <= lim
        assert np.array_equal(got[:, 12:], np.tile([0.0, 0.0, 0.0, 1.0], (len(xi), 1)))
