"""numpy restatement of core::interp_pose and core::transform (ouster_core/include/ouster/core/pose_util.h:118-173, :194-434;
src/transform_vector.cpp:40-60, 96-104; src/transform_homogeneous.cpp:31-62; impl/transform_typedefs.h:16-17), operation for
operation, in a dtype of the caller's choice: float64 is the arithmetic the library is held to, np.longdouble the truth the
tolerance tests measure both against (tests/golden/make_pose_golden.py).

Every sum runs left to right and no step is fused, so the float64 form is what csrc/host/pose_util.cpp and csrc/k_pose.hip
compute (both are built without FMA contraction) up to the library's sin / cos / acos.  The two inverses -- a.inverse() of the
full 4x4 and vee(...).inverse() of the 3x3 -- are general inverses by cofactors, as Eigen's fixed-size inverse is.

The segment of an x is defined per element: min(k - 2, #{j >= 1 : x_known[j] <= x}), which is what the reference's lower_bound
sweep gives for sorted x_interp (first / last segment extrapolate).  x_interp that decreases anywhere is refused: a superset
of where the reference throws (it checks inside a segment's run only)."""
import numpy as np

EPS = 2.0 ** -52            # std::numeric_limits<double>::epsilon()
NUMERIC_EPS = 2.0 ** -26    # std::sqrt(EPS)
DBL_EPSILON = EPS

MSG_FEW = "Not enough evaluation poses for interpolation"
MSG_SIZES = "x_known and poses_known sizes are not matching"
MSG_KNOWN = "input x_known values are not monotonically increasing or values repeated"
MSG_DURATION = "Cannot interpolate with zero duration between poses"
MSG_INTERP = "x_interp values must be monotonically increasing: "


def _mat(n, dt):
    return [[dt(0)] * n for _ in range(n)]


def matmul(a, b, n):
    """full n x n product, every sum left to right"""
    r = _mat(n, type(a[0][0]))
    for i in range(n):
        for j in range(n):
            s = a[i][0] * b[0][j]
            for k in range(1, n):
                s = s + a[i][k] * b[k][j]
            r[i][j] = s
    return r


def det3(m, rows, cols):
    a, b, c = rows
    p, q, r = cols
    return (m[a][p] * (m[b][q] * m[c][r] - m[b][r] * m[c][q]) - m[a][q] * (m[b][p] * m[c][r] - m[b][r] * m[c][p])
            + m[a][r] * (m[b][p] * m[c][q] - m[b][q] * m[c][p]))


def inv3(m):
    """general 3x3 inverse by cofactors: adjugate / determinant"""
    dt = type(m[0][0])
    cof = _mat(3, dt)
    for i in range(3):
        for j in range(3):
            r = [x for x in range(3) if x != i]
            c = [x for x in range(3) if x != j]
            minor = m[r[0]][c[0]] * m[r[1]][c[1]] - m[r[0]][c[1]] * m[r[1]][c[0]]
            cof[i][j] = minor if (i + j) % 2 == 0 else -minor
    det = m[0][0] * cof[0][0] + m[0][1] * cof[0][1] + m[0][2] * cof[0][2]
    return [[cof[j][i] / det for j in range(3)] for i in range(3)]


def inv4(m):
    """general 4x4 inverse by cofactors: adjugate / determinant"""
    dt = type(m[0][0])
    cof = _mat(4, dt)
    for i in range(4):
        for j in range(4):
            minor = det3(m, [x for x in range(4) if x != i], [x for x in range(4) if x != j])
            cof[i][j] = minor if (i + j) % 2 == 0 else -minor
    det = m[0][0] * cof[0][0] + m[0][1] * cof[0][1] + m[0][2] * cof[0][2] + m[0][3] * cof[0][3]
    return [[cof[j][i] / det for j in range(4)] for i in range(4)]


def skew(v):
    z = type(v[0])(0)
    return [[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]]


def vee(r, angle, sin_angle, cos_angle):
    """RotV::vee (transform_vector.cpp:52-60)"""
    dt = type(angle)
    one = dt(1)
    ident = [[one if i == j else dt(0) for j in range(3)] for i in range(3)]
    if angle < EPS:
        return ident
    a = skew([r[0] / angle, r[1] / angle, r[2] / angle])
    k1 = one - cos_angle
    k2 = angle - sin_angle
    t1 = [[(k1 * a[i][j]) / angle for j in range(3)] for i in range(3)]
    t2 = matmul([[k2 * a[i][j] for j in range(3)] for i in range(3)], a, 3)
    return [[(ident[i][j] + t1[i][j]) + t2[i][j] / angle for j in range(3)] for i in range(3)]


def pose_log(m):
    """PoseH::log (transform_homogeneous.cpp:31-62) of a 4x4: the 6 numbers rotation then translation"""
    dt = type(m[0][0])
    c = dt(0.5) * (((m[0][0] + m[1][1]) + m[2][2]) - dt(1))
    c = max(c, dt(-1) + dt(EPS))
    c = min(c, dt(1) - dt(EPS))
    angle = np.arccos(c)
    v = [m[2][1] - m[1][2], m[0][2] - m[2][0], m[1][0] - m[0][1]]
    sq = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    if sq > EPS:
        n = np.sqrt(sq)
        v = [(x / n) * angle for x in v]
    else:
        v = [x / dt(2) for x in v]
    s = np.sin(angle)
    vi = inv3(vee(v, angle, s, c))
    t = [m[0][3], m[1][3], m[2][3]]
    return v + [(vi[i][0] * t[0] + vi[i][1] * t[1]) + vi[i][2] * t[2] for i in range(3)]


def pose_exp(d):
    """PoseV::exp (transform_vector.cpp:40-50, 96-104): 4x4 with the bottom row 0 0 0 1"""
    dt = type(d[0])
    one, zero = dt(1), dt(0)
    r, t = d[:3], d[3:]
    angle = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    s, c = np.sin(angle), np.cos(angle)
    ident = [[one if i == j else zero for j in range(3)] for i in range(3)]
    if angle < NUMERIC_EPS:
        a = skew(r)
        rot = [[ident[i][j] + a[i][j] for j in range(3)] for i in range(3)]
    else:
        a = skew([r[0] / angle, r[1] / angle, r[2] / angle])
        k = one - c
        aa = matmul([[k * a[i][j] for j in range(3)] for i in range(3)], a, 3)
        rot = [[(ident[i][j] + s * a[i][j]) + aa[i][j] for j in range(3)] for i in range(3)]
    v = vee(r, angle, s, c)
    tr = [(v[i][0] * t[0] + v[i][1] * t[1]) + v[i][2] * t[2] for i in range(3)]
    return [rot[0] + [tr[0]], rot[1] + [tr[1]], rot[2] + [tr[2]], [zero, zero, zero, one]]


def _as_mat(p, dt):
    p = np.asarray(p, dtype=np.float64).reshape(4, 4)
    return [[dt(p[i, j]) for j in range(4)] for i in range(4)]


def segment(t0, x0, t1, x1, dtype=np.float64):
    """(t0, a as 4x4 lists, scaled_twist[6]) of one pair of known poses"""
    dt = dtype
    a, b = _as_mat(x0, dt), _as_mat(x1, dt)
    twist = pose_log(matmul(inv4(a), b, 4))
    f = dt(1) / (dt(t1) - dt(t0))
    return dt(t0), a, [f * x for x in twist]


def validate_known(x_known, poses_known):
    x_known = np.asarray(x_known, dtype=np.float64).reshape(-1)
    n_poses = len(poses_known)
    if x_known.size != n_poses:
        raise ValueError(MSG_SIZES)
    if x_known.size < 2:
        raise ValueError(MSG_FEW)
    for i in range(x_known.size - 1):
        if x_known[i] >= x_known[i + 1]:
            raise ValueError(MSG_KNOWN)
    return x_known


def validate_interp(x_interp):
    x = np.asarray(x_interp, dtype=np.float64).reshape(-1)
    for i in range(1, x.size):
        if x[i] < x[i - 1]:
            raise ValueError(MSG_INTERP + "%f < %f" % (x[i], x[i - 1]))
    return x


def segments_table(x_known, poses_known, dtype=np.float64):
    """[k - 1][24]: t0, a[16], scaled_twist[6], one pad -- the table ouster_hip_pose_segments writes"""
    x_known = validate_known(x_known, poses_known)
    out = np.zeros((x_known.size - 1, 24), dtype=dtype)
    for i in range(x_known.size - 1):
        t0, a, st = segment(x_known[i], poses_known[i], x_known[i + 1], poses_known[i + 1], dtype)
        out[i, 0] = t0
        out[i, 1:17] = [a[r][c] for r in range(4) for c in range(4)]
        out[i, 17:23] = st
    return out


def segment_index(x_known, x):
    """min(k - 2, #{j >= 1 : x_known[j] <= x})"""
    x_known = np.asarray(x_known, dtype=np.float64)
    return min(x_known.size - 2, int(np.count_nonzero(x_known[1:] <= x)))


def eval_segment(row, x):
    """one x on one row of the table, in the row's dtype: a @ exp((x - t0) * scaled_twist) as 16 numbers"""
    dt = row.dtype.type
    a = [[row[1 + 4 * r + c] for c in range(4)] for r in range(4)]
    d = dt(x) - row[0]
    m = matmul(a, pose_exp([d * row[17 + i] for i in range(6)]), 4)
    return [m[r][c] for r in range(4) for c in range(4)]


def interp_pose(x_interp, x_known, poses_known, dtype=np.float64, check_interp=True):
    """(N, 4, 4) of `dtype`"""
    table = segments_table(x_known, poses_known, dtype)
    x = validate_interp(x_interp) if check_interp else np.asarray(x_interp, dtype=np.float64).reshape(-1)
    out = np.zeros((x.size, 16), dtype=dtype)
    for i, xv in enumerate(x):
        out[i] = eval_segment(table[segment_index(x_known, xv)], xv)
    return out.reshape(-1, 4, 4)


def interp_pose_two(x_interp, t0, x0, t1, x1, dtype=np.float64):
    """the two-pose form (pose_util.h:316-326): any sign of t1 - t0, every x on the one segment"""
    if abs(float(t1) - float(t0)) < DBL_EPSILON:
        raise ValueError(MSG_DURATION)
    x = validate_interp(x_interp)
    t, a, st = segment(t0, x0, t1, x1, dtype)
    row = np.zeros(24, dtype=dtype)
    row[0] = t
    row[1:17] = [a[r][c] for r in range(4) for c in range(4)]
    row[17:23] = st
    out = np.zeros((x.size, 16), dtype=dtype)
    for i, xv in enumerate(x):
        out[i] = eval_segment(row, xv)
    return out.reshape(-1, 4, 4)


def transform(points, pose):
    """R p + t in the points' type, the pose cast to that type first (pose_util.h:118-131); any leading shape"""
    pts = np.asarray(points)
    dt = pts.dtype.type
    m = np.asarray(pose, dtype=np.float64).reshape(4, 4).astype(pts.dtype)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    out = np.empty_like(pts)
    for r in range(3):
        out[..., r] = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + dt(m[r, 3])
    return out


def bound(truth, model_err, scale):
    """what a result may differ from `truth` by, elementwise: 8 x the reference arithmetic's own error on the case, at least
    8 eps x scale -- a device sin / cos of 2 ulp against 1 ulp, carried through two 3x3 products and one 4x4 product"""
    del truth
    return 8.0 * max(1.0, float(model_err)) * EPS * float(scale)
