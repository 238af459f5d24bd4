"""algorithm::normals restated in float64, statement for statement (ouster_algorithm/src/normals.cpp): the yardstick of the GPU
form.  Plain Python floats (IEEE doubles): every multiply, add, subtract, divide and sqrt is rounded on its own, nothing is fused.

The reference's bit pattern depends on how Eigen was built (reduction order, contraction); this model's order is the definition:
    dot(a, b)      = (a0 * b0 + a1 * b1) + a2 * b2
    squaredNorm(a) = dot(a, a),   norm(a) = sqrt(squaredNorm(a))
    cross(a, b)    = (a1 * b2 - a2 * b1,  a2 * b0 - a0 * b2,  a0 * b1 - a1 * b0)
    v / s          = (v0 / s, v1 / s, v2 / s)            (a division per component, no reciprocal)
    2 pi r         = (2.0 * pi) * (range_mm * 0.001)
acos and tan are math.acos / math.tan (the host's libm) and occur only in per-call constants (constants()): the vertical subtent,
px_res = 2 pi / subtent for both axes and tan(max(min_angle, 1e-6)).

Clouds are (H * W, 3) or (H, W, 3), destaggered; the result is (H * W, 3) like the reference's MatrixX3dR."""
import math

import numpy as np

FOREGROUND_SALIENCE_MM = 500
DEFAULT_TARGET_DISTANCE_METER = 0.025
DEFAULT_MIN_ANGLE_INCIDENCE_RAD = 1 * math.pi / 180.0
EPS = 2.0 ** -52
INF = float("inf")

MSG_XYZ = "normals: xyz dimensions mismatch"
MSG_ORIGINS = "normals: sensor_origins size must match image width"
MSG_RANGE2 = "normals: range2 dimensions mismatch"
MSG_TARGET = "normals: target_distance_m must be positive"
MSG_ANGLE = "normals: min_angle_of_incidence_rad must be positive"

# which branch wrote a pixel (classify=True): what the GPU test's scene is checked for
ZERO_RANGE, CASE_A, CASE_B_VERTICAL, CASE_B_HORIZONTAL, CASE_C, CASE_C_FLIP, FELL_THROUGH = range(7)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _div(a, b):
    """IEEE division of doubles (Python raises where C++ gives inf / nan)"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return float("nan")
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def beam_of(p, o):
    d = (p[0] - o[0], p[1] - o[1], p[2] - o[2])
    m = math.sqrt(dot(d, d))
    if m > 0.0:
        return (d[0] / m, d[1] / m, d[2] / m)
    return (0.0, 0.0, 0.0)


def subtent_pair(xyz, rng, origins, h, w):
    """compute_vertical_subtent up to the acos: (dot of the two beams, unclamped, top - bottom) of the first column -- from W / 2
    outward, -offset then +offset -- whose highest and lowest rows with range differ; None where there is none."""
    mid = w // 2
    for off in range(mid + 1):
        for sign in (-1, 1):
            col = mid + sign * off
            if col < 0 or col >= w:
                continue
            top = h - 1 if h > 0 else 0
            bottom = 0
            while top > bottom:
                if rng[top * w + col] != 0 and rng[bottom * w + col] != 0:
                    return (dot(beam_of(xyz[top * w + col], origins[col]), beam_of(xyz[bottom * w + col], origins[col])),
                            top - bottom)
                t_ok, b_ok = rng[top * w + col] != 0, rng[bottom * w + col] != 0
                top -= 0 if t_ok else 1
                bottom += 0 if b_ok else 1
    return None


def vertical_subtent(h, pair):
    if pair is not None:
        d = pair[0]
        d = d if d < 1.0 else 1.0       # std::min(1.0, d): a NaN becomes 1.0
        d = d if -1.0 < d else -1.0     # std::max(-1.0, .)
        return math.acos(d) / float(pair[1])
    return (0.5 * math.pi) / float(max(1, h - 1))


def constants(w, h, min_angle_of_incidence_rad, target_distance_m, pair):
    """The per-call constants of compute_unit_normals; pair = (dot, top - bottom) or None (the 90 degree fallback)."""
    two_pi = 2.0 * math.pi
    subtent = vertical_subtent(h, pair)
    return {"px_res_h": _div(two_pi, _div(two_pi, float(w))), "px_res_v": _div(two_pi, subtent),
            "tan_safe": math.tan(max(min_angle_of_incidence_rad, 1e-6)), "target_sq": target_distance_m * target_distance_m,
            "subtent": subtent}


def _as_lists(xyz, rng, h, w):
    return (np.asarray(xyz, dtype=np.float64).reshape(h * w, 3).tolist(), np.asarray(rng).reshape(h * w).astype(np.int64).tolist())


def _unit_normals(xyz, rng, xyz2, rng2, h, w, origins, psr, min_angle, target, override=0.0, classify=None):
    if target <= 0.0:
        raise RuntimeError(MSG_TARGET)
    if min_angle <= 0.0:
        raise RuntimeError(MSG_ANGLE)
    pair = None
    if not override > 0.0:
        pair = subtent_pair(xyz, rng, origins, h, w)
        k = constants(w, h, min_angle, target, pair)
    else:
        k = constants(w, h, min_angle, target, None)
        k["subtent"] = override
        k["px_res_v"] = _div(2.0 * math.pi, override)
    px_res_h, px_res_v, tan_safe, target_sq = k["px_res_h"], k["px_res_v"], k["tan_safe"], k["target_sq"]
    dual = xyz2 is not None and rng2 is not None
    two_pi = 2.0 * math.pi
    out = [(0.0, 0.0, 0.0)] * (h * w)

    def threshold(range_mm, px_res):
        perimeter_m = two_pi * (float(range_mm) * 0.001)
        return _div(_div(perimeter_m, px_res), tan_safe)

    def find_best(vertical, u, v, nd_sq, center, center_range, max_up, max_down):
        """-> (found, diff, requires_flip, thin_foreground_flag)"""
        best_diff = (0.0, 0.0, 0.0)
        st = [INF, 1, False, True]   # min_distance_sq, best_radius, best_requires_flip, thin_foreground_flag
        good = False

        def consider(row, col, pts, rr, flip, radius):
            nonlocal best_diff
            i = row * w + col
            nr = rr[i]
            if nr == 0:
                return
            p = pts[i]
            d = (p[0] - center[0], p[1] - center[1], p[2] - center[2])
            dsq = dot(d, d)
            if nr - center_range < FOREGROUND_SALIENCE_MM:
                st[3] = False
            if abs(dsq - target_sq) < abs(st[0] - target_sq):
                best_diff = d
                st[0], st[1], st[2] = dsq, radius, flip

        for radius in range(1, psr + 1):
            if vertical and radius > max_up and radius > max_down:
                break
            if good and not st[3]:
                break
            if vertical:
                if radius <= max_up:
                    consider(u - radius, v, xyz, rng, True, radius)
                if radius <= max_down:
                    consider(u + radius, v, xyz, rng, False, radius)
                if dual:
                    if radius <= max_up:
                        consider(u - radius, v, xyz2, rng2, True, radius)
                    if radius <= max_down:
                        consider(u + radius, v, xyz2, rng2, False, radius)
            else:
                left = (int(math.fmod(v - radius, w)) + w) % w   # C's truncating %, then + W, then % W
                consider(u, left, xyz, rng, True, radius)
                if dual:
                    consider(u, left, xyz2, rng2, True, radius)
                right = (v + radius) % w
                consider(u, right, xyz, rng, False, radius)
                if dual:
                    consider(u, right, xyz2, rng2, False, radius)
            limit = (float(st[1]) * float(st[1])) * nd_sq
            if target_sq <= st[0] and st[0] < limit:
                good = True
            elif radius == psr:
                if st[0] > 0 and st[0] < limit:
                    good = True
        if good and st[0] < INF:
            return True, best_diff, st[2], st[3]
        return False, (0.0, 0.0, 0.0), False, st[3]

    def case_b(diff, beam):
        denom = dot(diff, diff)
        if abs(denom) < EPS:
            return None
        s = _div(dot(diff, beam), denom)
        pr = (beam[0] - s * diff[0], beam[1] - s * diff[1], beam[2] - s * diff[2])
        n_sq = dot(pr, pr)
        if abs(n_sq) < EPS:
            return None
        n = math.sqrt(n_sq)
        return (-(pr[0] / n), -(pr[1] / n), -(pr[2] / n))

    for u in range(h):
        max_up = min(psr, u)
        max_down = min(psr, h - 1 - u)
        for v in range(w):
            i = u * w + v
            center_range = rng[i]
            if center_range == 0:
                if classify is not None:
                    classify[i] = ZERO_RANGE
                continue
            if classify is not None:
                classify[i] = FELL_THROUGH
            center = xyz[i]
            beam = beam_of(center, origins[v])
            if dot(beam, beam) <= EPS:
                continue
            nd_h = threshold(center_range, px_res_h)
            nd_h_sq = nd_h * nd_h
            nd_v = threshold(center_range, px_res_v)
            nd_v_sq = nd_v * nd_v
            v_found, v_diff, v_flip, v_thin = find_best(True, u, v, nd_v_sq, center, center_range, max_up, max_down)
            h_found, h_diff, h_flip, h_thin = find_best(False, u, v, nd_h_sq, center, center_range, psr, psr)
            if (not v_found and not h_found) or (v_thin and h_thin):
                out[i] = (-beam[0], -beam[1], -beam[2])
                if classify is not None:
                    classify[i] = CASE_A
                continue
            if v_found and (not h_found or h_thin):
                n = case_b(v_diff, beam)
                if n is not None:
                    out[i] = n
                    if classify is not None:
                        classify[i] = CASE_B_VERTICAL
                continue
            elif h_found and (not v_found or v_thin):
                n = case_b(h_diff, beam)
                if n is not None:
                    out[i] = n
                    if classify is not None:
                        classify[i] = CASE_B_HORIZONTAL
                continue
            if h_flip != v_flip:
                v_diff = (-v_diff[0], -v_diff[1], -v_diff[2])
            n = cross(v_diff, h_diff)
            m = math.sqrt(dot(n, n))
            if m != 0.0:
                out[i] = (n[0] / m, n[1] / m, n[2] / m)
                if classify is not None:
                    classify[i] = CASE_C_FLIP if h_flip != v_flip else CASE_C
    return np.array(out, dtype=np.float64).reshape(h * w, 3)


def _shape_checks(xyz, rng):
    rng = np.asarray(rng)
    if rng.ndim != 2:
        raise TypeError("range must be a 2-D image")
    h, w = rng.shape
    xyz = np.asarray(xyz)
    if xyz.size != h * w * 3 or xyz.shape[-1] != 3:
        raise RuntimeError(MSG_XYZ)
    return h, w


def normals(xyz, range, xyz2=None, range2=None, *, sensor_origins_xyz=None, pixel_search_range=1,
            min_angle_of_incidence_rad=DEFAULT_MIN_ANGLE_INCIDENCE_RAD, target_distance_m=DEFAULT_TARGET_DISTANCE_METER,
            classify=False):
    """normals(xyz, range, sensor_origins_xyz=...) -> (H * W, 3);  normals(xyz, range, xyz2, range2, sensor_origins_xyz=...) -> a pair.
    classify=True appends the per-pixel branch codes (one (H * W,) int array per return)."""
    dual = xyz2 is not None or range2 is not None
    h, w = _shape_checks(xyz, range)
    if dual:
        x2 = np.asarray(xyz2)
        if x2.size != h * w * 3 or x2.shape[-1] != 3:
            raise RuntimeError(MSG_XYZ)
        if np.asarray(range2).shape != (h, w):
            raise RuntimeError(MSG_RANGE2)
    origins = np.asarray(sensor_origins_xyz, dtype=np.float64)
    if origins.ndim != 2 or origins.shape[1] != 3:
        raise TypeError("incompatible function arguments: sensor_origins_xyz must be (W, 3)")
    if origins.shape[0] != w:
        raise RuntimeError(MSG_ORIGINS)
    org = origins.tolist()
    psr = int(pixel_search_range)
    p1, r1 = _as_lists(xyz, range, h, w)
    if not dual:
        cls = [0] * (h * w) if classify else None
        n = _unit_normals(p1, r1, None, None, h, w, org, psr, min_angle_of_incidence_rad, target_distance_m, 0.0, cls)
        return (n, np.array(cls)) if classify else n
    p2, r2 = _as_lists(xyz2, range2, h, w)
    subtent = vertical_subtent(h, subtent_pair(p1, r1, org, h, w))
    c1 = [0] * (h * w) if classify else None
    c2 = [0] * (h * w) if classify else None
    first = _unit_normals(p1, r1, p2, r2, h, w, org, psr, min_angle_of_incidence_rad, target_distance_m, subtent, c1)
    second = _unit_normals(p2, r2, p1, r1, h, w, org, psr, min_angle_of_incidence_rad, target_distance_m, subtent, c2)
    return (first, second, np.array(c1), np.array(c2)) if classify else (first, second)


def sensor_origins(poses_w_by_16, sensor_to_body):
    """(W, 3): the translation of pose[c] * sensor_to_body, each entry a row times the last column, left to right:
    ((p0 * s03 + p1 * s13) + p2 * s23) + p3 * s33."""
    poses = np.asarray(poses_w_by_16, dtype=np.float64).reshape(-1, 16).tolist()
    s = np.asarray(sensor_to_body, dtype=np.float64).reshape(16).tolist()
    out = []
    for p in poses:
        out.append([((p[4 * r] * s[3] + p[4 * r + 1] * s[7]) + p[4 * r + 2] * s[11]) + p[4 * r + 3] * s[15] for r in (0, 1, 2)])
    return np.array(out, dtype=np.float64).reshape(-1, 3)
