"""The source of k_vmap_find, k_vmap_publish, k_vmap_admit, k_vmap_far, k_vmap_compact, k_vmap_rebuild, k_vmap_closest and
k_vmap_cloud (csrc/k_voxel_map.hip) run on the CPU, one thread per lane (tests/cpp/voxel_map_lanes.cpp over tests/cpp/host_lanes),
against tests/voxel_map_model.py bit for bit: index arithmetic and the order of the floating-point operations, without a GPU.
Shapes are small -- every lane is a thread -- but cross a workgroup, fill voxels across calls, wrap probe chains and evict."""
import struct
import subprocess

import numpy as np
import pytest

import cpp_tools
import voxel_map_cases as K
import voxel_map_model as M


def run_lanes(tmp_path, calls, queries, voxel_size, max_distance, max_points, bound_sq, origin, cap):
    case, result = tmp_path / "case.bin", tmp_path / "result.bin"
    queries = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
    with open(case, "wb") as f:
        f.write(struct.pack("<4I6d", len(calls), max_points, len(queries), cap, voxel_size, max_distance, bound_sq, *origin))
        for rows in calls:
            rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3)
            f.write(struct.pack("<2I", len(rows), 0))
            f.write(rows.tobytes())
        f.write(queries.tobytes())
    exe = cpp_tools.build("voxel_map_lanes")[0]
    p = subprocess.run([exe, str(case), str(result)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "voxel_map_lanes: done", (p.returncode, p.stdout, p.stderr)
    raw = open(result, "rb").read()
    status, voxels, points, kept = struct.unpack_from("<4I", raw, 0)
    at = 16
    cloud = np.frombuffer(raw, np.float64, points * 3, at).reshape(-1, 3)
    at += points * 24
    evicted, status2 = struct.unpack_from("<2I", raw, at)
    at += 8
    extracted = np.frombuffer(raw, np.float64, evicted * 3, at).reshape(-1, 3)
    at += evicted * 24
    after = np.frombuffer(raw, np.float64, (points - evicted) * 3, at).reshape(-1, 3)
    at += (points - evicted) * 24
    nn = np.frombuffer(raw, np.float64, len(queries) * 3, at).reshape(-1, 3)
    at += len(queries) * 24
    d2 = np.frombuffer(raw, np.float64, len(queries), at)
    assert at + len(queries) * 8 == len(raw) and status == 0 and status2 == 0
    return dict(voxels=voxels, points=points, kept=kept, cloud=cloud, extracted=extracted, after=after, nn=nn, d2=d2)


def check(tmp_path, calls, queries, voxel_size, max_distance, max_points, bound_sq, origin, cap):
    got = run_lanes(tmp_path, calls, queries, voxel_size, max_distance, max_points, bound_sq, origin, cap)
    model = M.VoxelHashMap3d(voxel_size, max_distance, max_points)
    for rows in calls:
        model.add_points(rows)
    assert (got["voxels"], got["points"]) == (model.num_voxels(), model.num_points())
    K.same_bytes(got["cloud"], model.pointcloud(), "cloud")
    K.same_bytes(got["extracted"], model.extract_voxels_far_from_location(origin), "extracted")
    assert got["kept"] == model.num_voxels()
    K.same_bytes(got["after"], model.pointcloud(), "cloud after the removal")
    want = model.get_closest_neighbors(queries, bound_sq)
    K.same_bytes(got["nn"], want[0], "neighbours")
    K.same_bytes(got["d2"], want[1], "distances")
    return got, model


def test_three_calls_a_removal_and_queries(tmp_path):
    rows = K.uniform_cloud(900, 3, extent=4.0)
    got, model = check(tmp_path, [rows[:300], rows[300:301], rows[250:]], K.uniform_cloud(300, 4, extent=4.5), 0.5, 2.0, 3, 0.3, (1.0, -0.5, 0.25), 2048)
    assert 0 < len(got["extracted"]) < got["points"] and (got["d2"] < 0.3).any() and (got["d2"] == 0.3).any()


def test_admission_boundary_ties_and_a_full_voxel(tmp_path):
    voxel, res_sq, held, at, nearer = K.admission_boundary(20)
    got, _ = check(tmp_path, [[held], [nearer, at], K.distant_in_one_voxel(60, voxel=8.0) + 16.0], [held, at, nearer], voxel, 1000.0, 20, M.DBL_MAX,
                   (0.0, 0.0, 0.0), 16)
    assert got["points"] == 2 + 20 and len(got["extracted"]) == 0
    pts, queries = K.lattice_ties()
    check(tmp_path, [pts], queries, 1.0, 100.0, 1, M.DBL_MAX, (0.0, 0.0, 0.0), 16)
    check(tmp_path, [pts], queries, 1.0, 100.0, 1, 0.75, (0.0, 0.0, 0.0), 16)      # d^2 == the bound is no match


def test_wrapping_chains_and_the_removal_boundary(tmp_path):
    cells = K.cells_starting_at(31, 31, 5) + K.cells_starting_at(30, 31, 4)
    rows = np.array([[c[0] + 0.5, c[1] + 0.5, c[2] + 0.5] for c in cells])
    check(tmp_path, [rows[:4], rows[2:], rows + 0.3], rows + 0.1, 1.0, 1e6, 2, 0.5, tuple(rows[0]), 16)      # 32 slots
    voxel, max_distance, rows, origin, cells = K.removal_boundary()
    got, _ = check(tmp_path, [rows], rows + 0.05, voxel, max_distance, 20, 1.0, origin, 16)
    assert len(got["extracted"]) == 6 and got["kept"] == 3


def test_the_edge_of_the_grid(tmp_path):
    top = float(2 ** 31 - 1)
    queries = [(top + 0.25, 0.5, 0.5), (float("nan"), 0.5, 0.5), (top + 1.5, 0.5, 0.5), (-top - 0.75, 0.5, 0.5)]
    got, _ = check(tmp_path, [[(top + 0.5, 0.5, 0.5), (top - 0.5, 0.5, 0.5), (-top - 0.5, 0.5, 0.5)]], queries, 1.0, 100.0, 20, 7.0, (top, 0.0, 0.0), 16)
    assert len(got["extracted"]) == 1       # the voxel 2^32 - 1 cells away: far, exactly
