"""CPU-only: tests/normals_model.py, the float64 restatement of algorithm::normals the GPU form is held to, is itself held to what
the reference recorded in its python/tests/test_normals.py: the two 2 x 2 regression arrays (single and dual), the five sample
pixels and the unit lengths on single_scan_016.osf, the six surfaces of the room scene (normals_test_data.osf) with the 0.5 degree
alignment rule, and the five error cases with their messages.

The inputs are built as that test builds them -- RANGE / RANGE2 of the first frame, XYZLut in double, destagger, zero origins --
from this project's pieces that need no GPU: the C++ container walk (core.OsfFile) and metadata reader (core.SensorInfo), the
pixel decode of the OSF oracle (the project's own plane decode is a kernel), and the oracle's XYZ tables (use_extrinsics as in
XYZLut's default), cartesian and destagger."""
import functools
import json
import os

import numpy as np
import pytest

import normals_model as M
from conftest import GOLDEN

OSF_DIR = os.path.join(GOLDEN, "osf")
CAR = os.path.join(OSF_DIR, "single_scan_016.osf")
ROOM = os.path.join(OSF_DIR, "normals_test_data.osf")


@functools.lru_cache(maxsize=None)
def osf_inputs(path):
    """-> h, w, shifts, {name: (destaggered xyz (h * w, 3) f64, destaggered range (h, w) u32)} for RANGE and RANGE2 (where present)"""
    from oracle import oracle as O
    from oracle import osf_oracle as Z
    from ouster_sdk_amd import core
    O.build()
    f = core.OsfFile(path)
    text = list(f.sensor_metadata_json().values())[0]
    meta = json.loads(text)
    df = meta.get("lidar_data_format") or meta["data_format"]
    h, w, shifts = df["pixels_per_column"], df["columns_per_frame"], df["pixel_shift_by_row"]
    streams = f.lidar_scan_streams()
    msg = [m for (_, sid, m) in f.messages() if sid in streams][0]
    fields = Z.decode_lidar_scan_msg(msg, h, w, shifts)["fields"]
    info = core.SensorInfo(text)
    extrinsic = (meta.get("ouster-sdk") or {}).get("extrinsic") or meta.get("extrinsic") or np.eye(4)
    transform = np.asarray(extrinsic, dtype=np.float64).reshape(4, 4) @ np.asarray(info.lidar_to_sensor_transform, dtype=np.float64)
    direction, offset = O.make_xyz_lut(w, h, 0.001, np.asarray(info.beam_to_lidar_transform), transform,
                                       np.asarray(info.beam_azimuth_angles), np.asarray(info.beam_altitude_angles))
    sh = np.array(shifts, np.int32)
    out = {}
    for name in ("RANGE", "RANGE2"):
        if name not in fields:
            continue
        rng = np.ascontiguousarray(fields[name], dtype=np.uint32)
        xyz = O.cartesian(rng, direction, offset).reshape(h, w, 3)
        out[name] = (O.destagger(xyz, sh).reshape(h * w, 3), O.destagger(rng, sh))
    return h, w, sh, out


@functools.lru_cache(maxsize=None)
def car_model():
    """the model on single_scan_016.osf: (single, first, second), each (h, w, 3); shared with the GPU test of the same scan"""
    h, w, _, d = osf_inputs(CAR)
    (xyz, rng), (xyz2, rng2) = d["RANGE"], d["RANGE2"]
    org = np.zeros((w, 3))
    single = M.normals(xyz, rng, sensor_origins_xyz=org)
    first, second = M.normals(xyz, rng, xyz2, rng2, sensor_origins_xyz=org)
    return tuple(a.reshape(h, w, 3) for a in (single, first, second))


X22 = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0], [1.0, 1.0, 0.0]]])
R22 = np.array([[0.0, 1.0], [1.0, 1.0]], np.uint32)
ARGS = dict(pixel_search_range=1, min_angle_of_incidence_rad=0.1, target_distance_m=100)


def test_reference_regression_arrays():
    want = np.array([[[0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], [[0.0, -1.0, 0.0], [-0.70710678, -0.70710678, 0.0]]])
    org = np.zeros((2, 3))
    assert np.allclose(M.normals(X22, R22, sensor_origins_xyz=org, **ARGS).reshape(2, 2, 3), want)
    first, second = M.normals(X22, R22, X22, R22, sensor_origins_xyz=org, **ARGS)
    assert np.allclose(first.reshape(2, 2, 3), want)
    x2 = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])
    r2 = np.array([[0.0, 1.0], [0.0, 0.0]], np.uint32)
    want2 = np.array([[[0.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0], [0, 0.0, 0.0]]])
    assert np.allclose(M.normals(x2, r2, sensor_origins_xyz=org, **ARGS).reshape(2, 2, 3), want2)
    first, second = M.normals(x2, r2, x2, r2, sensor_origins_xyz=org, **ARGS)
    assert np.allclose(first.reshape(2, 2, 3), want2)


def test_car_scan_sample_pixels_and_unit_length():
    single, first, second = car_model()
    for n in (single, first, second):
        norms = np.linalg.norm(n, axis=2)
        assert np.any(norms > 0)
        np.testing.assert_allclose(norms[norms > 0], 1.0, atol=1e-6)
    for (row, col), want in (((67, 798), [0.063, 0.998, -0.012]), ((68, 204), [0.025, -0.999, 0.028]),
                             ((100, 512), [-0.032, 0.017, 0.999])):
        np.testing.assert_allclose(single[row, col], want, atol=1e-3, rtol=0)
    for (row, col), want in (((58, 791), [-0.009, 0.983, -0.182]), ((46, 153), [0.569, -0.823, -0.007])):
        np.testing.assert_allclose(second[row, col], want, atol=1e-3, rtol=0)


def test_room_scene_surfaces():
    from oracle import oracle as O
    h, w, sh, d = osf_inputs(ROOM)
    xyz, rng = d["RANGE"]
    n = M.normals(xyz, rng, sensor_origins_xyz=np.zeros((w, 3))).reshape(h, w, 3)
    staggered = O.destagger(n, sh, inverse=True)
    surfaces = {
        "wall_pos_x": ([1, 127], [0, 1023], np.array([1.0, 0.0, 0.0])),
        "wall_neg_x": ([1, 127], [357, 667], np.array([-1.0, 0.0, 0.0])),
        "wall_pos_y": ([1, 127], [613, 923], np.array([0.0, 1.0, 0.0])),
        "wall_neg_y": ([1, 127], [101, 411], np.array([0.0, -1.0, 0.0])),
        "ceiling": ([0, 13], [0, 1023], np.array([0.0, 0.0, -1.0])),
        "floor": ([116, 127], [48, 1008], np.array([0.0, 0.0, 1.0])),
    }
    threshold = float(np.cos(np.deg2rad(0.5)))
    for name, ((r0, r1), (c0, c1), expected) in surfaces.items():
        region = staggered[r0:r1 + 1, c0:c1 + 1]
        assert region.size, name
        norms = np.linalg.norm(region, axis=-1)
        valid = norms > 0
        assert np.any(valid), name
        normalized = np.zeros_like(region)
        normalized[valid] = region[valid] / norms[valid, None]
        align = np.tensordot(normalized, expected, axes=([2], [0]))
        mask = (align > threshold) & valid
        assert np.any(mask), name
        assert np.min(np.tensordot(normalized[mask], expected, axes=([1], [0]))) > threshold, name


def test_error_cases_and_messages():
    org = np.zeros((2, 3))
    for extra in ((), (X22, R22)):
        with pytest.raises(RuntimeError, match="normals: target_distance_m must be positive"):
            M.normals(X22, R22, *extra, sensor_origins_xyz=org, pixel_search_range=1, min_angle_of_incidence_rad=0.017453292519943295,
                      target_distance_m=-100)
        with pytest.raises(RuntimeError, match="normals: min_angle_of_incidence_rad must be positive"):
            M.normals(X22, R22, *extra, sensor_origins_xyz=org, pixel_search_range=1, min_angle_of_incidence_rad=-0.1,
                      target_distance_m=100)
        with pytest.raises(RuntimeError, match="normals: sensor_origins size must match image width"):
            M.normals(X22, R22, *extra, sensor_origins_xyz=np.zeros((0, 3)), target_distance_m=100)
        with pytest.raises(RuntimeError, match="normals: xyz dimensions mismatch"):
            M.normals(X22, np.array([[0.0, 1.0]], np.uint32), *extra, sensor_origins_xyz=org, target_distance_m=100)
        with pytest.raises(TypeError, match="incompatible function arguments"):
            M.normals(X22, R22, *extra, sensor_origins_xyz=np.zeros((0, 0)), target_distance_m=100)
    with pytest.raises(RuntimeError, match="normals: range2 dimensions mismatch"):
        M.normals(X22, R22, X22, R22.reshape(1, 4), sensor_origins_xyz=org, target_distance_m=100)


def test_constants_and_origins():
    k = M.constants(1024, 128, M.DEFAULT_MIN_ANGLE_INCIDENCE_RAD, 0.025, None)
    assert k["subtent"] == (0.5 * np.pi) / 127.0 and k["target_sq"] == 0.025 * 0.025
    assert M.constants(8, 1, 0.1, 1.0, None)["subtent"] == 0.5 * np.pi
    assert M.constants(8, 4, 0.1, 1.0, (1.0 + 2.0 ** -52, 3))["subtent"] == 0.0      # the clamp
    assert M.constants(8, 4, 0.1, 1.0, (0.0, 2))["subtent"] == np.pi / 2 / 2
    rng = np.random.default_rng(3)
    poses = rng.normal(size=(5, 4, 4))
    s2b = rng.normal(size=(4, 4))
    got = M.sensor_origins(poses.reshape(5, 16), s2b)
    assert np.abs(got - np.stack([(p @ s2b)[:3, 3] for p in poses])).max() < 1e-14
