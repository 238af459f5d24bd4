"""tests/registration_model.py pinned by hand: values worked out on paper, not by the model.  CPU only."""
import math

import numpy as np

import registration_model as R
import voxel_map_model as M


def four_point_map():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    m = M.VoxelHashMap3d(0.5, 10.0)
    m.add_points(pts)
    return pts, m


def test_weight_at_zero_and_at_k():
    assert R.weight(0.0, 0.25) == 1.0            # k^2 / k^2
    assert R.weight(0.25, 0.25) == 0.25          # k^2 / (2 k)^2
    assert R.weight(3.0, 1.0) == 1.0 / 16.0


def test_one_correspondence_on_paper():
    # s = (1, 2, 3), q = (1, 2, 2): r = (0, 0, 1), r2 = 1, k = 1: w = 1 / 4
    t = dict(zip(R.SUMS, R.terms((1.0, 2.0, 3.0), (1.0, 2.0, 2.0), 1.0)))
    assert t["w"] == 0.25
    assert (t["wsx"], t["wsy"], t["wsz"]) == (0.25, 0.5, 0.75)
    assert t["j33"] == 0.25 * (4.0 + 9.0) and t["j44"] == 0.25 * (1.0 + 9.0) and t["j55"] == 0.25 * (1.0 + 4.0)
    assert (t["wsxsy"], t["wsxsz"], t["wsysz"]) == (0.5, 0.75, 1.5)
    assert (t["wrx"], t["wry"], t["wrz"]) == (0.0, 0.0, 0.25)
    assert (t["wcx"], t["wcy"], t["wcz"]) == (0.5, -0.25, 0.0)      # s x r = (2, -1, 0)
    sums, jtj, jtr = R.linear_system([tuple(t[k] for k in R.SUMS)])
    want = np.zeros((6, 6))
    want[0, 0] = want[1, 1] = want[2, 2] = 0.25
    want[3, 1], want[3, 2], want[4, 0], want[4, 2], want[5, 0], want[5, 1] = -0.75, 0.5, 0.75, -0.25, -0.5, 0.25
    want[3, 3], want[4, 3], want[4, 4], want[5, 3], want[5, 4], want[5, 5] = 3.25, -0.5, 2.5, -0.75, -1.5, 1.25
    assert np.array_equal(np.array(jtj), want)                       # the lower triangle; the upper stays zero
    assert jtr == [0.0, 0.0, 0.25, 0.5, -0.25, 0.0]


def test_folds_agree_on_exact_terms_and_differ_in_name_only():
    rows = [R.terms((1.0, 2.0, 3.0), (1.0, 2.0, 2.0), 1.0)] * 3 + [R.ZERO_TERMS]
    a = R.linear_system(rows, R.left_fold)[0]
    b = R.linear_system(rows, math.fsum)[0]
    assert a == b and a[0] == 0.75


def test_solve6_diagonal_and_zero_pivot():
    jtj = [[0.0] * 6 for _ in range(6)]
    for i, d in enumerate([2.0, 4.0, 0.0, 8.0, 1.0, 0.5]):
        jtj[i][i] = d
    jtj[0][5] = 123.0                                # the upper triangle is never read
    dx = R.solve6(jtj, [2.0, -4.0, 5.0, 8.0, 1.0, 1.0])
    assert dx == [-1.0, 1.0, 0.0, -1.0, -1.0, -2.0]   # the zero pivot gives a zero component
    assert R.solve6([[0.0] * 6 for _ in range(6)], [1.0] * 6) == [0.0] * 6


def test_solve6_against_numpy_on_a_dense_system():
    rng = np.random.default_rng(3)
    a = rng.normal(size=(6, 6))
    spd = a @ a.T + 6.0 * np.eye(6)
    b = rng.normal(size=6)
    dx = R.solve6(np.tril(spd).tolist(), b.tolist())
    assert np.allclose(dx, np.linalg.solve(spd, -b), rtol=1e-12, atol=1e-14)


def test_se3_exp_pure_translation():
    assert R.se3_exp([1.0, -2.0, 3.0, 0.0, 0.0, 0.0]) == (0.0, 0.0, 0.0, 1.0, 1.0, -2.0, 3.0)


def test_se3_exp_rotation_about_z():
    p = R.se3_exp([0.0, 0.0, 0.0, 0.0, 0.0, math.pi / 2])
    assert p[:2] == (0.0, 0.0) and p[4:] == (0.0, 0.0, 0.0)
    assert math.isclose(p[2], math.sqrt(0.5), rel_tol=4e-16) and math.isclose(p[3], math.sqrt(0.5), rel_tol=4e-16)
    moved = R.apply(p, (1.0, 0.0, 0.0))
    assert np.allclose(moved, (0.0, 1.0, 0.0), atol=4e-16)
    assert np.allclose(R.matrix(p)[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=4e-16)
    # with a translational part: t = V u, V of a quarter turn maps (1, 0, 0) to (2 / pi) (1, 1, 0)
    t = R.se3_exp([1.0, 0.0, 0.0, 0.0, 0.0, math.pi / 2])[4:]
    assert np.allclose(t, (2.0 / math.pi, 2.0 / math.pi, 0.0), atol=4e-16)


def test_se3_exp_small_angle_branch_at_its_threshold():
    below, at = 0.5e-10, 1e-10                       # theta^2 < eps^2 is strict
    p = R.se3_exp([1.0, 0.0, 0.0, 0.0, 0.0, below])
    assert p[3] == 1.0 and p[2] == 0.5 * below       # the Taylor factors round to 1 and 1 / 2
    assert p[4:] == (1.0, 0.5 * below, 0.0)          # V = I + hat(omega) / 2
    q = R.se3_exp([1.0, 0.0, 0.0, 0.0, 0.0, at])
    assert q[2] == math.sin(0.5 * at) / at * at and q[3] == math.cos(0.5 * at)


def test_compose_is_a_product_with_a_unit_quaternion():
    a = R.se3_exp([0.1, 0.2, -0.3, 0.3, -0.2, 0.1])
    b = R.se3_exp([-0.5, 0.0, 0.25, 0.0, 0.4, 0.0])
    c = R.compose(a, b)
    assert abs(math.sqrt(sum(x * x for x in c[:4])) - 1.0) <= 2.0 ** -52
    assert np.allclose(R.matrix(c), R.matrix(a) @ R.matrix(b), atol=1e-15)
    assert R.compose(R.IDENTITY, b) == b


def test_empty_map_no_iterations_and_no_correspondences():
    frame = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    assert R.align(frame, M.VoxelHashMap3d(0.5, 10.0), 5, 1e-4, 1.0, 0.1) == (R.IDENTITY, 0, 0, False)
    pts, m = four_point_map()
    assert R.align(pts, m, 0, 1e-4, 1.0, 0.1) == (R.IDENTITY, 0, 0, False)
    # nothing within reach: dx = 0, and the loop ends after one pass with the pose it has
    assert R.align(pts + 5.0, m, 7, 1e-4, 0.5, 0.1) == (R.IDENTITY, 1, 0, True)


def test_associate_is_strict_at_the_bound_and_skips_what_no_cell_holds():
    _, m = four_point_map()
    rows = [(0.25, 0.0, 0.0), (0.2, 0.0, 0.0), (float("nan"), 0.0, 0.0), (1e300, 0.0, 0.0)]
    got = R.associate(rows, m, 0.25)
    assert [f for f, _, _ in got] == [False, True, False, False]
    assert got[0][2] == 0.0625 and got[1][1] == (0.0, 0.0, 0.0)


def test_shifted_cloud_against_a_four_point_map_is_recovered():
    pts, m = four_point_map()
    shifted = pts + np.array([0.05, 0.02, -0.01])
    for fold in (R.left_fold, math.fsum):
        pose, passes, count, _ = R.align(shifted, m, 20, 1e-4, 0.5, 0.1, fold)
        T = R.matrix(pose)
        recovered = (T[:3, :3] @ shifted.T).T + T[:3, 3]
        assert np.allclose(recovered, pts, atol=0.05) and count == 4 and 1 <= passes <= 20
    # the moved cloud carries every pass's roundings: the loop's rows, not the frame moved by the composed pose
    trace = []
    R.align(shifted, m, 3, 0.0, 0.5, 0.1, trace=trace)
    assert len(trace) == 3


def test_adaptive_threshold_defaults_and_update():
    t = R.AdaptiveThreshold(100.0)
    assert (t.max_range, t.min_motion_threshold, t.compute_threshold()) == (100.0, 0.01, 2.0)
    t = R.AdaptiveThreshold(100.0, initial_threshold=1.0)
    dev = np.eye(4)
    dev[:3, 3] = [2.0, 0.0, 0.0]
    t.update_model_deviation(dev)
    assert t.num_samples == 2 and t.compute_threshold() == math.sqrt((1.0 + 4.0) / 2.0)
    small = np.eye(4)
    small[0, 3] = 0.01                               # exactly at min_motion_threshold: not a sample
    t.update_model_deviation(small)
    assert t.num_samples == 2


def test_rotation_angle_of_known_turns():
    c, s = math.cos(0.3), math.sin(0.3)
    assert math.isclose(R.rotation_angle([[c, -s, 0], [s, c, 0], [0, 0, 1]]), 0.3, rel_tol=1e-15)
    assert R.rotation_angle(np.eye(3)) == 0.0
    assert math.isclose(R.rotation_angle([[-1, 0, 0], [0, -1, 0], [0, 0, 1]]), math.pi, rel_tol=1e-15)   # trace <= 0: the other branch
    t = R.AdaptiveThreshold(10.0, 1.0)
    t.update_model_deviation([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert math.isclose(t.model_sse, 1.0 + (20.0 * math.sin(0.15)) ** 2, rel_tol=1e-14)
