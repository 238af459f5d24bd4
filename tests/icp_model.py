"""point_to_point_align / point_to_plane_align in float64, the yardstick of csrc/k_icp.hip and csrc/host/icp_util.cpp.

Restates ouster_algorithm/src/align_clouds.cpp:146-235 (median_abs, SpatialHashGrid3D), :1590-1874 (the two ICP loops) and
impl/spatial_hash.h operation by operation.  Eigen leaves the order of a few sums open; this file fixes it, and the code under
test follows this file:
  x    = ((r0*p0 + r1*p1) + r2*p2) + t   per row of the pose (R n likewise, without t)
  norm = sqrt((a*a + b*b) + c*c);  dot products and squared distances left to right
  cell = floor(p * (1.0 / max_corr_dist)) per axis
  outer products: (w * (x - cx)_i) * (q - cq)_j;  w * (j_a * j_b);  (-w) * (j_a * r)
  4x4 and 3x3 products: every entry a left-to-right sum (pose_model.matmul)
Every sum over correspondences comes in two forms: the reference's left fold in source order, and math.fsum (exact=True), which
bounds the GPU's reduction tree.  Two deviations, both stated in DESIGN section 5: a participating target coordinate whose cell no
int32 holds is refused, and a query whose cell lies outside the int32 grid has no neighbour.  The 3x3 SVD is a one-sided Jacobi
iteration and the 6x6 solve an LDL^T without pivoting, as in icp_util.cpp (Eigen: a two-sided Jacobi, a pivoted LDL^T)."""
import math

import numpy as np

import pose_model as P

MIN_ICP_POINTS = 20
MAD_TO_SIGMA = 1.4826
HUBER_K = 1.5
NORMAL_EPS = 1e-12
MAX_ITERATIONS = 10
POINT, PLANE = 0, 1

MSG_DIST = "max_corr_dist must be finite and greater than zero"
MSG_ANGLE = "max_normal_angle_deg must be finite and in [0, 180]"
MSG_SRC_ROWS = "source_points and source_normals must have the same number of rows"
MSG_TGT_ROWS = "target_points and target_normals must have the same number of rows"
MSG_ONE_SIDE = "normals must be given for both clouds or for neither"
MSG_GRID = ("point_to_point_align: target point outside the int32 cell grid",
            "point_to_plane_align: target point outside the int32 cell grid")
I32_MIN, I32_MAX = -2147483648.0, 2147483647.0
N_SUMS = 27    # point: w, w x (3), w q (3), then the 9 of the covariance (16 used); plane: 21 of the upper triangle, then 6


def validate(method, n_src, n_tgt, n_src_normals, n_tgt_normals, max_corr_dist, max_normal_angle_deg):
    """the reference's refusals in its order (align_clouds.cpp:1593-1595, 1731-1747)"""
    if not math.isfinite(max_corr_dist) or max_corr_dist <= 0.0:
        raise ValueError(MSG_DIST)
    if method == PLANE:
        if not math.isfinite(max_normal_angle_deg) or max_normal_angle_deg < 0.0 or max_normal_angle_deg > 180.0:
            raise ValueError(MSG_ANGLE)
        if n_src != n_src_normals:
            raise ValueError(MSG_SRC_ROWS)
        if n_tgt != n_tgt_normals:
            raise ValueError(MSG_TGT_ROWS)


def widen(a):
    """(n, >=3) of float32 / float64 -> (n, 3) float64, exactly"""
    a = np.asarray(a)
    return np.ascontiguousarray(a[:, :3], dtype=np.float64).reshape(-1, 3)


def norm3(a, b, c):
    return math.sqrt((a * a + b * b) + c * c)


def finite3(v):
    return math.isfinite(v[0]) and math.isfinite(v[1]) and math.isfinite(v[2])


def cos_gate(max_normal_angle_deg):
    return math.cos(max_normal_angle_deg * math.pi / 180.0)


class Grid:
    """SpatialHashGrid3D: cell -> the participating rows in ascending index"""

    def __init__(self, cells, inv):
        self.cells, self.inv = cells, inv


def build_grid(points, normals, cell, method=None):
    method = (PLANE if normals is not None else POINT) if method is None else method
    inv = 1.0 / cell
    cells = {}
    for j in range(len(points)):
        p = [float(v) for v in points[j]]
        if not finite3(p):
            continue
        if normals is not None:
            m = [float(v) for v in normals[j]]
            if not finite3(m) or norm3(m[0], m[1], m[2]) <= NORMAL_EPS:
                continue
        key = tuple(math.floor(v * inv) if math.isfinite(v * inv) else v * inv for v in p)
        if not all(I32_MIN <= k <= I32_MAX for k in key):
            raise ValueError(MSG_GRID[method])   # deviation: the reference keeps 64-bit cells
        cells.setdefault(tuple(int(k) for k in key), []).append(j)
    return Grid(cells, inv)


def nearest(grid, points, q, max_dist_sq):
    """SpatialHashGrid3D::nearest: 27 cells, dx outer, dz inner; rows of a cell in ascending index; strict < against a best that
    starts at max_dist_sq, so the first row in visiting order wins a tie and a row at exactly max_corr_dist is no match"""
    if not finite3(q) or not math.isfinite(max_dist_sq) or max_dist_sq <= 0.0:
        return -1
    f = [math.floor(v * grid.inv) if math.isfinite(v * grid.inv) else math.inf for v in q]
    if not all(I32_MIN <= k <= I32_MAX for k in f):
        return -1                                  # deviation: outside the int32 grid there is no neighbour
    c = [int(k) for k in f]
    best, best_d2 = -1, max_dist_sq
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                rows = grid.cells.get((c[0] + dx, c[1] + dy, c[2] + dz))   # a neighbour past the int32 range holds no row
                if not rows:
                    continue
                for j in rows:
                    p = points[j]
                    e0, e1, e2 = float(p[0]) - q[0], float(p[1]) - q[1], float(p[2]) - q[2]
                    d2 = (e0 * e0 + e1 * e1) + e2 * e2
                    if d2 < best_d2:
                        best_d2, best = d2, j
    return best


def rotate(pose, v, with_t):
    out = []
    for i in range(3):
        s = (pose[i][0] * v[0] + pose[i][1] * v[1]) + pose[i][2] * v[2]
        out.append(s + pose[i][3] if with_t else s)
    return out


def correspond(pose, src, tgt, src_n, tgt_n, grid, max_corr_dist, max_normal_angle_deg=20.0):
    """Per source row: nn (-1: none or gated out), r (0.0 where nn < 0), x, and q (point) or the unit target normal (plane)."""
    n = len(src)
    plane = src_n is not None
    nn = np.full(n, -1, np.int32)
    r = np.zeros(n)
    xs, qs = np.zeros((n, 3)), np.zeros((n, 3))
    d2max = max_corr_dist * max_corr_dist
    gate = cos_gate(max_normal_angle_deg) if plane else 0.0
    pose = [[float(v) for v in row] for row in np.asarray(pose).reshape(4, 4)]
    for i in range(n):
        p = [float(v) for v in src[i]]
        if plane:
            m = [float(v) for v in src_n[i]]
            length = norm3(m[0], m[1], m[2])
            if not finite3(m) or length <= NORMAL_EPS:
                continue
            m = [m[0] / length, m[1] / length, m[2] / length]
        x = rotate(pose, p, True)
        j = nearest(grid, tgt, x, d2max)
        if j < 0:
            continue
        q = [float(v) for v in tgt[j]]
        e = [x[0] - q[0], x[1] - q[1], x[2] - q[2]]
        if plane:
            mw = rotate(pose, m, False)
            t = [float(v) for v in tgt_n[j]]
            length = norm3(t[0], t[1], t[2])
            if not finite3(t) or length <= NORMAL_EPS:
                continue
            t = [t[0] / length, t[1] / length, t[2] / length]
            align = abs((t[0] * mw[0] + t[1] * mw[1]) + t[2] * mw[2])
            if not math.isfinite(align) or align < gate:
                continue
            res = (t[0] * e[0] + t[1] * e[1]) + t[2] * e[2]
            second = t
        else:
            res = norm3(e[0], e[1], e[2])
            second = q
        if not math.isfinite(res):
            continue
        nn[i], r[i] = j, res
        xs[i], qs[i] = x, second
    return nn, r, xs, qs


def median_abs(values):
    v = sorted(abs(float(x)) for x in values)
    if not v:
        return 0.0
    mid = len(v) // 2
    return v[mid] if len(v) & 1 else 0.5 * (v[mid - 1] + v[mid])


def huber_delta(mad, max_corr_dist):
    sigma = MAD_TO_SIGMA * mad
    if not math.isfinite(sigma) or sigma < 1e-4:
        sigma = max(1e-3, 0.25 * max_corr_dist)
    return HUBER_K * sigma


def weight(r, delta):
    a = abs(r)
    return 1.0 if (a <= delta or delta <= 0.0) else delta / a


def terms_point_a(nn, r, xs, qs, delta):
    """(m, 7): w, w x, w q of the rows with a correspondence, in source order"""
    out = []
    for i in np.flatnonzero(nn >= 0):
        w = weight(float(r[i]), delta)
        out.append([w] + [w * float(v) for v in xs[i]] + [w * float(v) for v in qs[i]])
    return np.array(out).reshape(-1, 7)


def terms_point_b(nn, r, xs, qs, delta, cx, cq):
    """(m, 9): (w (x - cx)_i) (q - cq)_j, row-major"""
    out = []
    for i in np.flatnonzero(nn >= 0):
        w = weight(float(r[i]), delta)
        wx = [w * (float(xs[i][k]) - cx[k]) for k in range(3)]
        dq = [float(qs[i][k]) - cq[k] for k in range(3)]
        out.append([wx[a] * dq[b] for a in range(3) for b in range(3)])
    return np.array(out).reshape(-1, 9)


UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def terms_plane(nn, r, xs, ns, delta):
    """(m, 27): w (j_a j_b) for a <= b row-major, then (-w) (j_a r), with j = (x cross n, n)"""
    out = []
    for i in np.flatnonzero(nn >= 0):
        res = float(r[i])
        w = weight(res, delta)
        x, m = [float(v) for v in xs[i]], [float(v) for v in ns[i]]
        j = [x[1] * m[2] - x[2] * m[1], x[2] * m[0] - x[0] * m[2], x[0] * m[1] - x[1] * m[0], m[0], m[1], m[2]]
        out.append([w * (j[a] * j[b]) for a, b in UPPER] + [(-w) * (j[a] * res) for a in range(6)])
    return np.array(out).reshape(-1, 27)


def fold(terms, exact):
    """the reference's left fold from zero in source order, or the exact sum rounded once"""
    if exact:
        return [math.fsum(terms[:, k]) for k in range(terms.shape[1])]
    s = [0.0] * terms.shape[1]
    for row in terms.tolist():
        s = [a + b for a, b in zip(s, row)]
    return s


def svd3(a):
    """One-sided Jacobi on the columns of a 3x3: (u, sigma, v) with a = u diag(sigma) v^T, sigma descending, u's third column the
    cross product of the first two, signed like a's third column; None where the second singular value is zero or not finite (no rotation is determined)."""
    a = [row[:] for row in a]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(30):
        rotated = False
        for p, q in ((0, 1), (0, 2), (1, 2)):
            alpha = (a[0][p] * a[0][p] + a[1][p] * a[1][p]) + a[2][p] * a[2][p]
            beta = (a[0][q] * a[0][q] + a[1][q] * a[1][q]) + a[2][q] * a[2][q]
            gamma = (a[0][p] * a[0][q] + a[1][p] * a[1][q]) + a[2][p] * a[2][q]
            if gamma == 0.0 or not abs(gamma) > P.EPS * math.sqrt(alpha * beta):
                continue
            rotated = True
            zeta = (beta - alpha) / (2.0 * gamma)
            t = math.copysign(1.0, zeta) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = c * t
            for m in (a, v):
                for i in range(3):
                    mp, mq = m[i][p], m[i][q]
                    m[i][p] = c * mp - s * mq
                    m[i][q] = s * mp + c * mq
        if not rotated:
            break
    sigma = [norm3(a[0][k], a[1][k], a[2][k]) for k in range(3)]
    order = sorted(range(3), key=lambda k: -sigma[k]) if all(math.isfinite(s) for s in sigma) else None
    if order is None or not sigma[order[1]] > 0.0:
        return None
    sigma = [sigma[k] for k in order]
    a = [[a[i][k] for k in order] for i in range(3)]
    v = [[v[i][k] for k in order] for i in range(3)]
    u = [[a[i][0] / sigma[0], a[i][1] / sigma[1], 0.0] for i in range(3)]
    u[0][2] = u[1][0] * u[2][1] - u[2][0] * u[1][1]
    u[1][2] = u[2][0] * u[0][1] - u[0][0] * u[2][1]
    u[2][2] = u[0][0] * u[1][1] - u[1][0] * u[0][1]
    if (u[0][2] * a[0][2] + u[1][2] * a[1][2]) + u[2][2] * a[2][2] < 0.0:     # the side the third column of a lies on
        u[0][2], u[1][2], u[2][2] = -u[0][2], -u[1][2], -u[2][2]
    return u, sigma, v


def det3(m):
    return ((m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]))
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def solve_point(cov, cx, cq):
    """Kabsch with the determinant fix: (4x4 delta, d_rot, d_trans) or None"""
    usv = svd3(cov)
    if usv is None:
        return None
    u, _, v = usv
    ut = [[u[j][i] for j in range(3)] for i in range(3)]
    rot = P.matmul(v, ut, 3)
    if det3(rot) < 0.0:
        v = [[v[i][0], v[i][1], -v[i][2]] for i in range(3)]
        rot = P.matmul(v, ut, 3)
    t = [cq[i] - ((rot[i][0] * cx[0] + rot[i][1] * cx[1]) + rot[i][2] * cx[2]) for i in range(3)]
    if not all(math.isfinite(x) for row in rot for x in row) or not finite3(t):
        return None
    delta = [rot[0] + [t[0]], rot[1] + [t[1]], rot[2] + [t[2]], [0.0, 0.0, 0.0, 1.0]]
    trace_term = max(-1.0, min(0.5 * (((rot[0][0] + rot[1][1]) + rot[2][2]) - 1.0), 1.0))
    return delta, math.acos(trace_term), norm3(t[0], t[1], t[2])


def ldlt6(h, b):
    """h x = b for a symmetric positive definite 6x6 by L D L^T without pivoting; None where a pivot is not positive"""
    n = 6
    low = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    for j in range(n):
        s = h[j][j]
        for k in range(j):
            s = s - (low[j][k] * low[j][k]) * d[k]
        if not s > 0.0 or not math.isfinite(s):
            return None
        d[j] = s
        low[j][j] = 1.0
        for i in range(j + 1, n):
            s = h[i][j]
            for k in range(j):
                s = s - (low[i][k] * low[j][k]) * d[k]
            low[i][j] = s / d[j]
    y = [0.0] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s = s - low[i][k] * y[k]
        y[i] = s
    x = [0.0] * n
    for i in reversed(range(n)):
        s = y[i] / d[i]
        for k in range(i + 1, n):
            s = s - low[k][i] * x[k]
        x[i] = s
    return x if all(math.isfinite(v) for v in x) else None


def solve_plane(sums):
    """one Gauss-Newton step: (4x4 delta, d_rot, d_trans) or None"""
    h = [[0.0] * 6 for _ in range(6)]
    for k, (a, b) in enumerate(UPPER):
        h[a][b] = h[b][a] = sums[k]
    for a in range(6):
        h[a][a] = h[a][a] + 1e-10
    dx = ldlt6(h, list(sums[21:27]))
    if dx is None:
        return None
    delta = [[float(v) for v in row] for row in P.pose_exp([float(v) for v in dx])]
    return delta, norm3(dx[0], dx[1], dx[2]), norm3(dx[3], dx[4], dx[5])


def step(method, pose, src, tgt, src_n, tgt_n, grid, max_corr_dist, max_normal_angle_deg=20.0, exact=False):
    """One pass of the loop from `pose`.  stop: the loop ends after this pass; solved: it had at least 20 correspondences."""
    pose = [[float(v) for v in row] for row in np.asarray(pose, dtype=np.float64).reshape(4, 4)]
    nn, r, xs, qs = correspond(pose, src, tgt, src_n if method == PLANE else None, tgt_n if method == PLANE else None, grid,
                               max_corr_dist, max_normal_angle_deg)
    count = int((nn >= 0).sum())
    out = dict(nn=nn, r=r, x=xs, q=qs, count=count, median=0.0, huber_delta=0.0, sums=[0.0] * N_SUMS, centroid_x=[0.0] * 3,
               centroid_q=[0.0] * 3, next_pose=pose, stop=True, solved=False, terms_a=None, terms_b=None)
    if count < MIN_ICP_POINTS:
        return out
    out["solved"] = True
    out["median"] = median_abs(r[nn >= 0])
    delta = out["huber_delta"] = huber_delta(out["median"], max_corr_dist)
    if method == POINT:
        out["terms_a"] = terms_point_a(nn, r, xs, qs, delta)
        a = fold(out["terms_a"], exact)
        out["sums"][:7] = a
        if not math.isfinite(a[0]) or a[0] <= 1e-12:
            return out
        cx = out["centroid_x"] = [a[1] / a[0], a[2] / a[0], a[3] / a[0]]
        cq = out["centroid_q"] = [a[4] / a[0], a[5] / a[0], a[6] / a[0]]
        out["terms_b"] = terms_point_b(nn, r, xs, qs, delta, cx, cq)
        b = fold(out["terms_b"], exact)
        out["sums"][7:16] = b
        solved = solve_point([b[0:3], b[3:6], b[6:9]], cx, cq)
    else:
        out["terms_a"] = terms_plane(nn, r, xs, qs, delta)
        out["sums"] = fold(out["terms_a"], exact)
        solved = solve_plane(out["sums"])
    if solved is None:
        return out
    delta_pose, d_rot, d_trans = solved
    out["next_pose"] = P.matmul(delta_pose, pose, 4)
    out["stop"] = d_rot < 1e-4 and d_trans < 1e-3
    return out


def align(method, src, tgt, src_n=None, tgt_n=None, initial_guess=None, max_corr_dist=0.25, max_normal_angle_deg=20.0, exact=False,
          trace=None):
    """-> (pose (4, 4), iterations, correspondences of the last pass, solved).  iterations counts the passes of the loop that
    were run, the one that ended it included.  trace: a list that receives every pass's step()."""
    guess = np.eye(4) if initial_guess is None else np.array(initial_guess, dtype=np.float64).reshape(4, 4)
    src, tgt = np.asarray(src), np.asarray(tgt)
    validate(method, len(src), len(tgt), len(src_n) if src_n is not None else 0, len(tgt_n) if tgt_n is not None else 0,
             max_corr_dist, max_normal_angle_deg)
    if len(src) < MIN_ICP_POINTS or len(tgt) < MIN_ICP_POINTS:
        return guess.copy(), 0, 0, False
    src, tgt = widen(src), widen(tgt)
    if method == PLANE:
        src_n, tgt_n = widen(src_n), widen(tgt_n)
    grid = build_grid(tgt, tgt_n if method == PLANE else None, max_corr_dist, method)
    pose, solved, iterations, count = guess.tolist(), False, 0, 0
    for _ in range(MAX_ITERATIONS):
        s = step(method, pose, src, tgt, src_n, tgt_n, grid, max_corr_dist, max_normal_angle_deg, exact)
        if trace is not None:
            trace.append(s)
        iterations, count = iterations + 1, s["count"]
        solved = solved or s["solved"]
        pose = s["next_pose"]
        if s["stop"]:
            break
    return (np.array(pose) if solved else guess.copy()), iterations, count, solved


def point_to_point_align(source_points, target_points, initial_guess=None, max_corr_dist=0.25, **kw):
    return align(POINT, source_points, target_points, None, None, initial_guess, max_corr_dist, **kw)[0]


def point_to_plane_align(source_points, target_points, source_normals, target_normals, initial_guess=None, max_corr_dist=0.25,
                         max_normal_angle_deg=20.0, **kw):
    return align(PLANE, source_points, target_points, source_normals, target_normals, initial_guess, max_corr_dist,
                 max_normal_angle_deg, **kw)[0]
