"""Writes tests/golden/pose_vectors.npz: the cases the interp_pose tolerance tests run (tests/test_pose_api_cpu.py,
tests/test_gpu_pose.py, tests/test_gpu_pose_batch.py use the same bound).  Per case `c`:
    c/x_known (k,), c/poses_known (k, 16), c/x_interp (n,)       the inputs, float64
    c/truth (n, 12)      rows 0..2 of tests/pose_model.py in np.longdouble, rounded to double (every known pose here has the
                         bottom row 0 0 0 1, and so has every result, exactly)
    c/scale              max(1, max |element| of the known poses and of truth)
    c/model_err          max |model_float64 - truth| / (eps * scale): the reference arithmetic's own error on the case
    c/table_truth (k - 1, 24), c/table_scale, c/table_err        the same three for the per-segment table (t0 is exact)
A result passes when |got - truth| <= 8 * max(1, model_err) * eps * scale elementwise (pose_model.bound).

Conditions on the inputs (the log is ill-conditioned near 0 and near pi, and the reference's clamp turns angles between about
7e-9 and 2e-8 into 2.1e-8): relative rotations are exactly 0, at most 1e-9 rad, or in [0.05, 2.5] rad; translations up to
1e3 m (the 1e-9 rad case: positions up to 1e3 m, 1 mm apart); times near 1.7e9 s, 0.05 - 1 s apart; extrapolation at most one segment length.  The maker asserts model_err <= 64 for
every case: a case that breaks it gets other inputs, never a higher cap.

Run from the repository root:  python tests/golden/make_pose_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pose_model as M  # noqa: E402

CAP = 64.0


def rodrigues(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def trajectory(rng, k, rel_angle, t_scale=1e3):
    """k poses (k, 16): every pose's rotation is the one before times a rotation by rel_angle(i) about a random axis"""
    rot = rodrigues(rng.normal(size=3), rng.uniform(0.1, 3.0))
    poses = []
    for i in range(k):
        if i:
            ang = rel_angle(i)
            if ang != 0.0:
                rot = rot @ rodrigues(rng.normal(size=3), ang)
        m = np.eye(4)
        m[:3, :3] = rot
        m[:3, 3] = rng.uniform(-t_scale, t_scale, size=3)
        poses.append(m.reshape(16))
    return np.array(poses)


def times(rng, k):
    return 1.7e9 + rng.uniform(0, 100) + np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 1.0, size=k - 1))])


def x_values(rng, xk, n):
    """sorted: before the first known time, on every known time, inside every segment, after the last, the rest anywhere"""
    first, last = xk[1] - xk[0], xk[-1] - xk[-2]
    xs = [xk[0] - first, xk[0] - 0.37 * first, xk[-1] + 0.61 * last, xk[-1] + last] + list(xk)
    for i in range(len(xk) - 1):
        xs += list(xk[i] + (xk[i + 1] - xk[i]) * np.array([0.001, 0.5, 0.999]))
    xs = xs[:n] if len(xs) > n else xs + list(rng.uniform(xk[0] - first, xk[-1] + last, size=n - len(xs)))
    return np.sort(np.array(xs, dtype=np.float64))


def main():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        raise SystemExit("np.longdouble is not wider than double here: the truth cannot be made on this machine")
    rng = np.random.default_rng(20240917)
    cases = {}
    for k in (2, 3, 9):
        cases["k%d" % k] = (times(rng, k), trajectory(rng, k, lambda i: rng.uniform(0.05, 2.5)), 257)
    cases["translation"] = (times(rng, 3), trajectory(rng, 3, lambda i: 0.0), 17)
    # a relative rotation of 1e-9 rad: cos(angle) rounds to 1 in double, so vee() drops its (1 - cos) / angle = angle / 2 term and
    # the double arithmetic is off by angle / 2 x the relative translation.  Under the cap that allows millimetres here, not
    # kilometres: the two poses sit near 1e3 m and 1 mm apart
    tiny = trajectory(rng, 2, lambda i: 1e-9)
    tiny[1, 3::4][:3] = tiny[0, 3::4][:3] + rng.uniform(-1e-3, 1e-3, size=3)
    cases["tiny"] = (times(rng, 2), tiny, 17)
    out = {}
    worst = 0.0
    eps = M.EPS
    for name, (xk, poses, n) in cases.items():
        xi = x_values(rng, xk, n)
        truth_l = M.interp_pose(xi, xk, poses, np.longdouble)
        truth = truth_l.astype(np.float64)
        model = M.interp_pose(xi, xk, poses, np.float64)
        assert np.array_equal(truth[:, 3, :], np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))
        scale = max(1.0, float(np.abs(poses).max()), float(np.abs(truth).max()))
        err = float(np.abs(model - truth).max() / (eps * scale))
        tab_truth = M.segments_table(xk, poses, np.longdouble).astype(np.float64)
        tab = M.segments_table(xk, poses, np.float64)
        assert np.array_equal(tab[:, 0], tab_truth[:, 0])
        tscale = max(1.0, float(np.abs(tab_truth[:, 1:]).max()))
        terr = float(np.abs(tab - tab_truth)[:, 1:].max() / (eps * tscale))
        print("%-12s k %d n %3d scale %.3g model_err %.2f table_err %.2f" % (name, len(xk), n, scale, err, terr))
        assert err <= CAP and terr <= CAP, "change the inputs of this case, not the cap"
        worst = max(worst, err)
        out.update({name + "/x_known": xk, name + "/poses_known": poses, name + "/x_interp": xi,
                    name + "/truth": truth.reshape(n, 16)[:, :12].copy(), name + "/scale": np.float64(scale),
                    name + "/model_err": np.float64(err), name + "/table_truth": tab_truth,
                    name + "/table_scale": np.float64(tscale), name + "/table_err": np.float64(terr)})
    path = os.path.join(HERE, "pose_vectors.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("largest model_err %.2f; %s: %d bytes" % (worst, path, size))
    assert size < 100 * 1024


if __name__ == "__main__":
    main()
