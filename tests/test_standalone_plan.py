"""CPU-only: the launch plan of the standalone kernels (ouster_sdk_amd/csrc/standalone_plan.cpp) against tables written by
hand from the launchers (now in k_destagger.hip, k_cartesian.hip and k_dewarp.hip) as they stood before the plan became a unit
of its own.

tools/standalone_plan_tool.cpp -- g++ only, no HIP library -- evaluates plan_destagger / plan_cartesian / plan_dewarp; every
expected value below was worked out on paper from these rules, not taken from the tool:

  destagger   al = row_bytes % 16 == 0 and both pointers 16 B aligned
              al and rows_env != 0 and row_bytes <= (16 KB if rows_env > 0 else 4 KB):
                  k_destagger_rows<CH>, CH from ceil(row_bytes / 16 / 256) -> 1 | 2 | 4, rows_per_wg = rows_env > 0 ? rows_env : 2,
                  LDS = 2 rows, grid = (ceil(h / rows_per_wg), n)
              else k_destagger on grid (h, n): LDS = the row if al and row_bytes <= 64 KB (LDS), 0 if al (DIRECT), 0 (BYTES)
  tiled       (cartesian: vec_ok and w % 4 == 0; dewarp: aligned and w % 4 == 0)
              tiles = ceil(w / tile); rpb = h, halved (rounding up) while rpb > 16 and tiles * n * ceil(h / rpb) < 1024,
              then rounded up to a multiple of 16; grid.x = tiles * ceil(h / rpb)
              cartesian: images_per_block doubles from 1 while 2 * ipb <= min(16, n) and grid.x * ceil(n / (2 * ipb)) >= 2048;
              grid.y = ceil(n / ipb) (dewarp: n)
  generic     grid = min(8192, max(1, ceil(items / 256))), items = ceil(w * h / 4) * n (cartesian) or w * h * n (dewarp)
"""
import subprocess

import pytest

import standalone_plan_query as Q

# (row_bytes, aligned, rows_env, h, n) -> (route, rows_per_wg, lds_bytes, grid)
DESTAGGER = [
    # the default (OUSTER_HIP_DESTAGGER_ROWS not set): two rows per workgroup up to 4 KB rows
    ((1024, 1, -1, 5, 3), ("ROWS1", 2, 2048, [3, 3])),
    ((2048, 1, -1, 128, 4), ("ROWS1", 2, 4096, [64, 4])),
    ((16, 1, -1, 1, 1), ("ROWS1", 2, 32, [1, 1])),
    ((4096, 1, -1, 5, 3), ("ROWS1", 2, 8192, [3, 3])),        # the last row size of the rows route
    ((4097, 1, -1, 5, 3), ("BYTES", 1, 0, [5, 3])),           # not 16 B granular
    ((4112, 1, -1, 5, 3), ("LDS", 1, 4112, [5, 3])),          # the first 16 B granular row past 4 KB
    ((8192, 1, -1, 5, 3), ("LDS", 1, 8192, [5, 3])),
    ((12288, 1, -1, 3, 3), ("LDS", 1, 12288, [3, 3])),
    ((65536, 1, -1, 5, 3), ("LDS", 1, 65536, [5, 3])),        # the last row that fits the LDS budget
    ((65537, 1, -1, 5, 3), ("BYTES", 1, 0, [5, 3])),
    ((65552, 1, -1, 5, 3), ("DIRECT", 1, 0, [5, 3])),         # the first that does not
    ((98304, 1, -1, 3, 3), ("DIRECT", 1, 0, [3, 3])),
    # row_bytes % 16 != 0, or a pointer off alignment: byte by byte whatever the size
    ((999, 1, -1, 5, 3), ("BYTES", 1, 0, [5, 3])),
    ((4008, 1, -1, 5, 3), ("BYTES", 1, 0, [5, 3])),
    ((6000, 1, -1, 3, 3), ("LDS", 1, 6000, [3, 3])),          # 16 B granular, not a power of two
    ((1024, 0, -1, 5, 3), ("BYTES", 1, 0, [5, 3])),
    ((4096, 0, -1, 5, 3), ("BYTES", 1, 0, [5, 3])),
    ((8192, 0, -1, 5, 3), ("BYTES", 1, 0, [5, 3])),
    ((98304, 0, -1, 3, 3), ("BYTES", 1, 0, [3, 3])),
    # rows_env = 0: never k_destagger_rows
    ((1024, 1, 0, 5, 3), ("LDS", 1, 1024, [5, 3])),
    ((4096, 1, 0, 5, 3), ("LDS", 1, 4096, [5, 3])),
    ((65552, 1, 0, 5, 3), ("DIRECT", 1, 0, [5, 3])),
    ((4096, 0, 0, 5, 3), ("BYTES", 1, 0, [5, 3])),
    # rows_env = 3: three rows per workgroup, up to 16 KB rows; 256 chunks of 16 B per CH
    ((1024, 1, 3, 7, 1), ("ROWS1", 3, 2048, [3, 1])),
    ((4096, 1, 3, 7, 1), ("ROWS1", 3, 8192, [3, 1])),
    ((4112, 1, 3, 7, 1), ("ROWS2", 3, 8224, [3, 1])),
    ((8192, 1, 3, 7, 3), ("ROWS2", 3, 16384, [3, 3])),
    ((8208, 1, 3, 7, 1), ("ROWS4", 3, 16416, [3, 1])),
    ((12288, 1, 3, 6, 2), ("ROWS4", 3, 24576, [2, 2])),
    ((16384, 1, 3, 7, 3), ("ROWS4", 3, 32768, [3, 3])),      # the last row size of the rows route under the variable
    ((16400, 1, 3, 7, 1), ("LDS", 1, 16400, [7, 1])),
    ((65552, 1, 3, 7, 1), ("DIRECT", 1, 0, [7, 1])),
    ((4096, 0, 3, 7, 1), ("BYTES", 1, 0, [7, 1])),
    ((4097, 1, 3, 7, 1), ("BYTES", 1, 0, [7, 1])),
    # rows_env = 1: one row per workgroup through the pipelined kernel
    ((4096, 1, 1, 5, 3), ("ROWS1", 1, 8192, [5, 3])),
]

# (w, h, n, vec_ok, tile) -> (route, tile_width, rows_per_block, images_per_block, grid)
CARTESIAN = [
    # small batches: the rows are split until 1024 workgroups exist or 16 rows are left
    ((1024, 128, 3, 1, 64), ("TILED", 64, 16, 1, [128, 3])),
    ((1024, 100, 30, 1, 64), ("TILED", 64, 32, 1, [64, 30])),     # 100 -> 50 -> 25 rows, rounded up to 32
    ((68, 20, 1, 1, 64), ("TILED", 64, 16, 1, [4, 1])),
    ((68, 20, 8, 1, 64), ("TILED", 64, 16, 1, [4, 8])),
    ((36, 7, 2, 1, 64), ("TILED", 64, 16, 1, [1, 2])),
    # the ladder of images per workgroup at h=20, w=68 (2 tiles x 1 row chunk of 32 rows): step k needs ceil(n / k) >= 1024
    ((68, 20, 2046, 1, 64), ("TILED", 64, 32, 1, [2, 2046])),
    ((68, 20, 2047, 1, 64), ("TILED", 64, 32, 2, [2, 1024])),
    ((68, 20, 4092, 1, 64), ("TILED", 64, 32, 2, [2, 2046])),
    ((68, 20, 4093, 1, 64), ("TILED", 64, 32, 4, [2, 1024])),
    ((68, 20, 8184, 1, 64), ("TILED", 64, 32, 4, [2, 2046])),
    ((68, 20, 8185, 1, 64), ("TILED", 64, 32, 8, [2, 1024])),
    ((68, 20, 16368, 1, 64), ("TILED", 64, 32, 8, [2, 2046])),
    ((68, 20, 16369, 1, 64), ("TILED", 64, 32, 16, [2, 1024])),
    ((68, 20, 16391, 1, 64), ("TILED", 64, 32, 16, [2, 1025])),
    ((68, 20, 40000, 1, 64), ("TILED", 64, 32, 16, [2, 2500])),   # 16 at most
    # the group is also bounded by the batch: 1024 tiles, three images
    ((65536, 128, 3, 1, 64), ("TILED", 64, 128, 2, [1024, 2])),
    # the benchmark's sizes: 256 images of 128 x 2048 (32 tiles: 4 per workgroup) and of 128 x 1024 (16 tiles: 2)
    ((2048, 128, 256, 1, 64), ("TILED", 64, 128, 4, [32, 64])),
    ((1024, 128, 256, 1, 64), ("TILED", 64, 128, 2, [16, 128])),
    # 256-column tiles (OUSTER_HIP_CT_TILE=256)
    ((1024, 128, 256, 1, 256), ("TILED", 256, 128, 1, [4, 256])),
    # the generic kernel: a width that is no multiple of 4, or vec_ok false
    ((33, 4, 2, 1, 64), ("GENERIC", 0, 0, 1, [1, 1])),
    ((36, 7, 2, 0, 64), ("GENERIC", 0, 0, 1, [1, 1])),
    ((1024, 128, 3, 0, 64), ("GENERIC", 0, 0, 1, [384, 1])),
    ((1001, 128, 100, 1, 64), ("GENERIC", 0, 0, 1, [8192, 1])),   # 12513 blocks of quads, capped
    ((1, 1, 1, 0, 64), ("GENERIC", 0, 0, 1, [1, 1])),
]

# (w, h, n, aligned, tile) -> (route, tile_width, rows_per_block, grid)
DEWARP = [
    ((512, 64, 3, 1, 64), ("TILED", 64, 16, [32, 3])),
    ((36, 7, 3, 1, 64), ("TILED", 64, 16, [1, 3])),
    ((1024, 100, 1, 1, 64), ("TILED", 64, 16, [112, 1])),         # 100 -> 50 -> 25 -> 13 rows
    ((1024, 100, 30, 1, 64), ("TILED", 64, 32, [64, 30])),
    ((2048, 128, 256, 1, 64), ("TILED", 64, 128, [32, 256])),
    ((2048, 128, 256, 1, 256), ("TILED", 256, 128, [8, 256])),
    ((36, 7, 3, 0, 64), ("GENERIC", 0, 0, [3, 1])),
    ((1001, 33, 2, 1, 64), ("GENERIC", 0, 0, [259, 1])),
    ((1001, 128, 100, 1, 64), ("GENERIC", 0, 0, [8192, 1])),
    ((1, 1, 1, 0, 64), ("GENERIC", 0, 0, [1, 1])),
]


def test_standalone_plan_tool_links_no_hip_library():
    out = subprocess.run(["ldd", Q.TOOL], capture_output=True, text=True).stdout.lower()
    assert "hip" not in out and "hsa" not in out, out


def test_destagger_plans():
    got = Q.query(Q.destagger_line(*i) for i, _ in DESTAGGER)
    bad = [(i, want, (g["route"], g["rows_per_wg"], g["lds_bytes"], g["grid"]))
           for (i, want), g in zip(DESTAGGER, got) if (g["route"], g["rows_per_wg"], g["lds_bytes"], g["grid"]) != want]
    assert not bad, bad


def test_cartesian_plans():
    got = Q.query(Q.cartesian_line(*i) for i, _ in CARTESIAN)
    key = lambda g: (g["route"], g["tile_width"], g["rows_per_block"], g["images_per_block"], g["grid"])
    bad = [(i, want, key(g)) for (i, want), g in zip(CARTESIAN, got) if key(g) != want]
    assert not bad, bad


def test_dewarp_plans():
    got = Q.query(Q.dewarp_line(*i) for i, _ in DEWARP)
    key = lambda g: (g["route"], g["tile_width"], g["rows_per_block"], g["grid"])
    bad = [(i, want, key(g)) for (i, want), g in zip(DEWARP, got) if key(g) != want]
    assert not bad, bad
    assert all(g["images_per_block"] == 1 for g in got)


def test_tables_cover_what_they_must():
    rows = {(i[0], i[2]) for i, _ in DESTAGGER if i[1]}
    assert {(4096, -1), (4097, -1), (65536, -1), (65552, -1)} <= rows                      # each boundary at its exact edge
    assert {i[2] for i, _ in DESTAGGER} >= {-1, 0, 3}
    assert any(i[0] % 16 for i, _ in DESTAGGER) and any(not i[1] for i, _ in DESTAGGER)
    assert {o[0] for _, o in DESTAGGER} == {"ROWS1", "ROWS2", "ROWS4", "LDS", "DIRECT", "BYTES"}
    ladder = {}
    for i, o in CARTESIAN:
        if i[:2] == (68, 20) and o[0] == "TILED":
            ladder.setdefault(o[3], []).append(i[2])
    for step in (2, 4, 8, 16):                              # the smallest batch of each step, and one image fewer one step below
        assert min(ladder[step]) - 1 in ladder[step // 2], step
    assert {o[0] for _, o in CARTESIAN} == {"TILED", "GENERIC"} == {o[0] for _, o in DEWARP}


def test_smallest_n_for_group_finds_the_ladder():
    assert [Q.smallest_n_for_group(68, 20, k) for k in (2, 4, 8, 16)] == [2047, 4093, 8185, 16369]


def test_tool_rejects_an_incomplete_query():
    r = subprocess.run([Q.TOOL], input="cartesian w=68 h=20 n=3\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "bad query" in r.stderr


@pytest.mark.parametrize("bad", ["destagger row_bytes=16 aligned=1 rows_env=-1 h=1 n=1 tile=64", "dewarp w=4 h=1 n=1 vec_ok=1 tile=64"])
def test_tool_rejects_a_name_of_another_form(bad):
    r = subprocess.run([Q.TOOL], input=bad + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
