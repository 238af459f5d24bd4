"""The yardstick of the frame-to-map registration: the reference's mapping::ICPRegistration::align_points_to_map
(ouster_mapping/src/icp_registration.cpp, include/ouster/mapping/icp_registration.h) and mapping::AdaptiveThreshold
(adaptive_threshold.cpp / .h) restated stage by stage in Python floats: every multiply, add, subtract, divide and sqrt below is one
IEEE double operation, in the order written here.  The device (csrc/k_registration.hip) and the host half
(csrc/host/registration_util.cpp) are held to this file.

Deviations from the reference, all of them about what it leaves open:
  * the solve.  The reference calls Eigen's pivoting LDLT, which this project cannot build or check against (no Eigen).  solve6
    is one L D L^T without pivoting, columns left to right, reading the lower triangle only, in the order written below.  Eigen's
    rule that a zero pivot gives a zero component is kept (so a pass without correspondences gives dx = 0);
  * the sums.  The reference reduces with TBB's deterministic reduce over blocks of 128 correspondences; linear_system takes the
    fold as an argument (the left fold for the host form, math.fsum as the exact yardstick) and the device uses the fixed tree of
    csrc/k_icp.hip.  The terms that are summed are the same everywhere;
  * rounding orders Eigen leaves to its vectoriser are fixed: a squared norm is ((x x + y y) + z z), a cross product component is
    a_y b_z - a_z b_y, a quaternion's rotation of a vector is (v + w uv) + (q x uv) with uv = 2 (q x v), the quaternion product
    and the norm it is renormalised by are spelled out in compose();
  * se3_exp follows the published form of Sophus's SE3::exp (unit quaternion from sin(theta / 2) / theta and cos(theta / 2), the
    Taylor branch below theta^2 < 1e-20, V = leftJacobian); it is not pose_exp of csrc/host/pose_util.cpp, which builds a rotation
    matrix by Rodrigues' formula and has the rotational part first;
  * a row that is non-finite or outside the int32 voxel grid has no correspondence (the reference's behaviour is undefined there).

The system of one pass is described by 16 sums and the integer count (SUMS below): the three w entries of the diagonal are one
sum, and the six hat(s) entries of the bottom-left block are plus or minus three sums; negation is exact."""
import math

import numpy as np

EPS = 1e-10   # Sophus::Constants<double>::epsilon()

# the 16 sums of a pass, in the order the device keeps them
SUMS = ("w", "wsx", "wsy", "wsz", "j33", "wsxsy", "j44", "wsxsz", "wsysz", "j55", "wrx", "wry", "wrz", "wcx", "wcy", "wcz")
N_SUMS = 16


# ---- association
def associate(moved, map_model, max_distance):
    """data_association: per row (flag, neighbour, squared distance), input order kept.  flag iff the squared distance the map
    returns is strictly below max_distance^2."""
    bound = max_distance * max_distance
    out = []
    for p in moved:
        q, d2 = map_model.get_closest_neighbor(p, bound)
        out.append((d2 < bound, q, d2))
    return out


# ---- the terms of one correspondence
def weight(r2, kernel_scale):
    """Geman-McClure: k^2 / (k + r2)^2"""
    k = kernel_scale
    return (k * k) / ((k + r2) * (k + r2))


def terms(source, target, kernel_scale):
    """what build_linear_system adds for one correspondence: the 16 entries of SUMS"""
    sx, sy, sz = (float(c) for c in source)
    rx, ry, rz = sx - float(target[0]), sy - float(target[1]), sz - float(target[2])
    r2 = (rx * rx + ry * ry) + rz * rz
    w = weight(r2, kernel_scale)
    wsx, wsy, wsz = w * sx, w * sy, w * sz
    wsx2, wsy2, wsz2 = wsx * sx, wsy * sy, wsz * sz
    cx, cy, cz = sy * rz - sz * ry, sz * rx - sx * rz, sx * ry - sy * rx   # s x r, the cross product first
    return (w, wsx, wsy, wsz,
            wsy2 + wsz2, wsx * sy, wsx2 + wsz2, wsx * sz, wsy * sz, wsx2 + wsy2,
            w * rx, w * ry, w * rz,
            w * cx, w * cy, w * cz)


ZERO_TERMS = (0.0,) * N_SUMS   # what a row without a correspondence adds


def left_fold(values):
    v = 0.0
    for x in values:
        v = v + x
    return v


def system_of_sums(sums):
    """the 16 sums -> (jtj [6][6] with the lower triangle filled and the upper left zero, jtr [6])"""
    s = dict(zip(SUMS, sums))
    jtj = [[0.0] * 6 for _ in range(6)]
    jtj[0][0] = jtj[1][1] = jtj[2][2] = s["w"]
    jtj[3][1], jtj[3][2] = -s["wsz"], s["wsy"]
    jtj[4][0], jtj[4][2] = s["wsz"], -s["wsx"]
    jtj[5][0], jtj[5][1] = -s["wsy"], s["wsx"]
    jtj[3][3] = s["j33"]
    jtj[4][3], jtj[4][4] = -s["wsxsy"], s["j44"]
    jtj[5][3], jtj[5][4], jtj[5][5] = -s["wsxsz"], -s["wsysz"], s["j55"]
    jtr = [s["wrx"], s["wry"], s["wrz"], s["wcx"], s["wcy"], s["wcz"]]
    return jtj, jtr


def linear_system(term_rows, fold=left_fold):
    """-> (sums [16], jtj, jtr) of the rows of terms, each sum folded by `fold` (left_fold or math.fsum) in input order"""
    term_rows = list(term_rows)
    sums = [float(fold([t[k] for t in term_rows])) for k in range(N_SUMS)]
    jtj, jtr = system_of_sums(sums)
    return sums, jtj, jtr


# ---- the solve
def solve6(jtj, jtr):
    """dx = solve(jtj, -jtr): L D L^T without pivoting, the lower triangle only.  A zero pivot gives a zero column of L and a zero
    component."""
    n = 6
    L = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    for j in range(n):
        v = jtj[j][j]
        for k in range(j):
            v = v - (L[j][k] * L[j][k]) * d[k]
        d[j] = v
        for i in range(j + 1, n):
            a = jtj[i][j]
            for k in range(j):
                a = a - (L[i][k] * L[j][k]) * d[k]
            L[i][j] = a / v if v != 0.0 else 0.0
    y = [0.0] * n
    for i in range(n):           # L y = -jtr
        a = -jtr[i]
        for k in range(i):
            a = a - L[i][k] * y[k]
        y[i] = a
    for i in range(n):           # D z = y
        y[i] = y[i] / d[i] if d[i] != 0.0 else 0.0
    x = [0.0] * n
    for i in range(n - 1, -1, -1):   # L^T x = z
        a = y[i]
        for k in range(i + 1, n):
            a = a - L[k][i] * x[k]
        x[i] = a
    return x


# ---- SE(3): a pose is (qx, qy, qz, qw, tx, ty, tz)
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def se3_exp(dx):
    """Sophus SE3::exp: dx = (upsilon, omega), the translational part first"""
    ux, uy, uz, ox, oy, oz = (float(c) for c in dx)
    theta_sq = (ox * ox + oy * oy) + oz * oz
    if theta_sq < EPS * EPS:
        theta_po4 = theta_sq * theta_sq
        imag = (0.5 - (1.0 / 48.0) * theta_sq) + (1.0 / 3840.0) * theta_po4
        real = (1.0 - (1.0 / 8.0) * theta_sq) + (1.0 / 384.0) * theta_po4
        a, b = 0.5, 0.0            # V = I + 0.5 hat(omega)
    else:
        theta = math.sqrt(theta_sq)
        half = 0.5 * theta
        imag = math.sin(half) / theta
        real = math.cos(half)
        a = (1.0 - math.cos(theta)) / theta_sq
        b = (theta - math.sin(theta)) / (theta_sq * theta)
    q = (imag * ox, imag * oy, imag * oz, real)
    # t = V u = u + a (omega x u) + b (omega x (omega x u))
    o, u = (ox, oy, oz), (ux, uy, uz)
    c1 = cross(o, u)
    c2 = cross(o, c1)
    t = tuple((u[k] + a * c1[k]) + b * c2[k] for k in range(3))
    return q + t


def rotate(q, v):
    """the unit quaternion's rotation of a vector: v + w uv + q x uv with uv = 2 (q x v)"""
    qv = (q[0], q[1], q[2])
    uv = cross(qv, v)
    uv = (uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2])
    c = cross(qv, uv)
    return tuple((v[k] + q[3] * uv[k]) + c[k] for k in range(3))


def apply(pose, p):
    """pose * point"""
    r = rotate(pose, (float(p[0]), float(p[1]), float(p[2])))
    return (r[0] + pose[4], r[1] + pose[5], r[2] + pose[6])


def compose(a, b):
    """a * b: the quaternion product renormalised by its norm, t = t_a + R_a t_b"""
    ax, ay, az, aw = a[:4]
    bx, by, bz, bw = b[:4]
    w = ((aw * bw - ax * bx) - ay * by) - az * bz
    x = ((aw * bx + ax * bw) + ay * bz) - az * by
    y = ((aw * by + ay * bw) + az * bx) - ax * bz
    z = ((aw * bz + az * bw) + ax * by) - ay * bx
    n = math.sqrt(((x * x + y * y) + z * z) + w * w)
    r = rotate(a, b[4:7])
    return (x / n, y / n, z / n, w / n, a[4] + r[0], a[5] + r[1], a[6] + r[2])


def matrix(pose):
    """SE3::matrix(): the rotation matrix of the quaternion (Eigen's toRotationMatrix) and the translation, 4 x 4"""
    x, y, z, w = pose[:4]
    tx, ty, tz = x + x, y + y, z + z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy, pose[4]],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx, pose[5]],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy), pose[6]],
                     [0.0, 0.0, 0.0, 1.0]])


# ---- one pass and the loop
def one_pass(moved, estimate, map_model, max_distance, kernel_scale, fold=left_fold, sums_override=None):
    """applies `estimate` (None: nothing) to the rows of `moved` in place, associates, sums, solves.
    -> dict(flags, neighbours, dist_sq, terms, sums, count, dx, estimate)"""
    if estimate is not None:
        for i, p in enumerate(moved):
            moved[i] = apply(estimate, p)
    assoc = associate(moved, map_model, max_distance)
    rows = [terms(p, q, kernel_scale) if f else ZERO_TERMS for p, (f, q, _) in zip(moved, assoc)]
    sums, jtj, jtr = linear_system(rows, fold)
    if sums_override is not None:
        sums = list(sums_override)
        jtj, jtr = system_of_sums(sums)
    dx = solve6(jtj, jtr)
    return dict(flags=[f for f, _, _ in assoc], neighbours=[q for _, q, _ in assoc], dist_sq=[d for _, _, d in assoc], terms=rows,
                sums=sums, count=sum(1 for f, _, _ in assoc if f), dx=dx, estimate=se3_exp(dx))


def squared_norm6(dx):
    return ((((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]) + dx[3] * dx[3]) + dx[4] * dx[4]) + dx[5] * dx[5]


def align(frame, map_model, max_iterations=50, convergence=1e-4, max_distance=1.0, kernel_scale=0.1, fold=left_fold, trace=None):
    """align_points_to_map_impl.  -> (pose, passes run, correspondences of the last pass, converged).  trace: a list that gets every
    pass's dict."""
    if map_model.empty() or max_iterations <= 0:
        return IDENTITY, 0, 0, False
    moved = [tuple(float(c) for c in p) for p in np.asarray(frame, dtype=np.float64).reshape(-1, 3)]
    pose, estimate, passes, count, converged = IDENTITY, None, 0, 0, False
    for _ in range(max_iterations):
        p = one_pass(moved, estimate, map_model, max_distance, kernel_scale, fold)
        if trace is not None:
            trace.append(p)
        estimate = p["estimate"]
        pose = compose(estimate, pose)
        passes, count = passes + 1, p["count"]
        if squared_norm6(p["dx"]) < convergence * convergence:
            converged = True
            break
    return pose, passes, count, converged


# ---- AdaptiveThreshold
def rotation_angle(R):
    """Eigen's AngleAxisd(R).angle(): the matrix to a quaternion, then 2 atan2(|vec|, |w|)"""
    m = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    t = (m[0][0] + m[1][1]) + m[2][2]
    q = [0.0, 0.0, 0.0]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q = [(m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t]
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(((m[i][i] - m[j][j]) - m[k][k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    n = math.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    return 2.0 * math.atan2(n, abs(w)) if n != 0.0 else 0.0


class AdaptiveThreshold:
    def __init__(self, max_range, initial_threshold=2.0, min_motion_threshold=0.01):
        self.min_motion_threshold = float(min_motion_threshold)
        self.max_range = float(max_range)
        self.model_sse = float(initial_threshold) * float(initial_threshold)
        self.num_samples = 1

    def update_model_deviation(self, deviation):
        d = np.asarray(deviation, dtype=np.float64).reshape(4, 4)
        theta = rotation_angle(d[:3, :3])
        delta_rot = (2.0 * self.max_range) * math.sin(theta / 2.0)
        tx, ty, tz = float(d[0, 3]), float(d[1, 3]), float(d[2, 3])
        delta_trans = math.sqrt((tx * tx + ty * ty) + tz * tz)
        model_error = delta_trans + delta_rot
        if model_error > self.min_motion_threshold:
            self.model_sse = self.model_sse + model_error * model_error
            self.num_samples += 1

    def compute_threshold(self):
        return math.sqrt(self.model_sse / float(self.num_samples))
