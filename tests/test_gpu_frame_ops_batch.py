"""frame_ops on a resident hip::DeviceFrameBatch, through tests/cpp/frame_ops_batch_tool.cpp: 5 frames of two sensors (different
LUTs and masks) decoded from encoded packets; RANGE and REFLECTIVITY also destaggered, XYZ in double, the dewarp gate counted by
the decode.  After every op everything the batch holds -- staggered planes, destaggered copies, both clouds -- must equal the
numpy model of tests/frame_ops_model.py applied to what was downloaded BEFORE the op, bit for bit; fields an op does not name
stay as they were.  The tool itself compares the clouds with the C ABI's cartesian of the filtered range planes; dewarp(gate)
after the RANGE filters must return the model's point list, which shows that the decode's gate counts were dropped.

The batch destaggers every frame with the first sensor's pixel_shift_by_row (decode() does), so the two sensors here share
their shifts.  Guard bands around device planes are checked on the C ABI level (tests/test_gpu_frame_ops.py): a batch owns
its allocations and exposes nothing around them."""
import math

import numpy as np
import pytest

import cpp_tools
import frame_ops_model as M
from conftest import has_gpu

pytestmark = pytest.mark.gpu

H, W, N = 32, 512, 5
SECOND = M.SECOND_RETURN_FIELDS


def tool_shifts(h, w):
    """make_info(h, w, variant, wrap_shifts = true) of tests/cpp/batch_fixture.h"""
    out = []
    for i in range(h):
        az = [4.2, 1.4, -1.4, -4.2][i % 4]
        s = int(np.rint(az / 360.0 * w))
        out.append(s + (w if i == 1 else 0) - (2 * w if i == 2 else 0))
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def nontrivial(inv):
    frac = float(np.mean(inv))
    assert 0.05 <= frac <= 0.95, f"the model invalidates {frac:.3f} of the pixels: the case shows nothing"


@pytest.fixture(scope="module")
def run(oracle, tmp_path_factory):
    assert has_gpu()
    O = oracle
    tmp = tmp_path_factory.mktemp("fops_batch")
    cal = O.synthetic_calib(h=H, w=W, profile="RNG15_RFL8_NIR8_DUAL")
    packets, frames = O.synth_packets(cal, N, zero_range_frac=0.1)
    np.ascontiguousarray(packets).tofile(tmp / "packets.bin")
    rng = np.random.default_rng(11)
    masks = np.stack([(rng.integers(0, 4, (H, W)) > 0).astype(np.uint8) * 9, np.ones((H, W), np.uint8)])
    masks[1, :, : W // 3] = 0
    masks.tofile(tmp / "masks.bin")
    r = np.stack([f.plane("RANGE") for f in frames])
    nz = r[r > 0]
    p = dict(clip_lo=float(np.percentile(nz, 15)), clip_hi=float(np.percentile(nz, 85)), key_lo=40.0, key_hi=90.0,
             gate_min=float(np.percentile(nz, 5)) / 1000.0, gate_max=float(np.percentile(nz, 95)) / 1000.0)
    # a band around z = 0 sized from the data: about a third of the live points by r * sin(altitude) (the tool's beam angles),
    # plus the points earlier ops have already put at the origin
    alt = np.deg2rad(21.0 - 42.0 * np.arange(H) / (H - 1.0))
    z = np.abs(r.astype(np.float64) * 1e-3 * np.sin(alt)[None, :, None])
    band = float(np.percentile(z[r > 0], 30))
    p["z_lo"], p["z_hi"] = -band, band
    args = [tmp / "packets.bin", H, W, N, tmp / "masks.bin", tmp / "o"] + \
           [repr(p[k]) for k in ("clip_lo", "clip_hi", "key_lo", "key_hi", "gate_min", "gate_max", "z_lo", "z_hi")]
    res = cpp_tools.run("frame_ops_batch_tool", args)
    layout = [(ln.split()[1], int(ln.split()[2])) for ln in res.stdout.splitlines() if ln.startswith("plane ")]
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

    def load(k):
        raw = np.fromfile(tmp / ("o.s%d" % k), np.uint8)
        off, st = 0, {"planes": {}, "dst": {}, "xyz": []}
        for name, es in layout:
            n = N * H * W * es
            st["planes"][name] = raw[off:off + n].view(dt[es]).reshape(N, H, W).copy()
            off += n
        for name in ("RANGE", "REFLECTIVITY"):
            es = dict(layout)[name]
            n = N * H * W * es
            st["dst"][name] = raw[off:off + n].view(dt[es]).reshape(N, H, W).copy()
            off += n
        for _ in range(2):
            n = N * H * W * 24
            st["xyz"].append(raw[off:off + n].view(np.float64).reshape(N, H * W, 3).copy())
            off += n
        assert off == raw.size
        return st
    stages = [load(k) for k in range(7)]
    return dict(stdout=res.stdout, stages=stages, params=p, masks=masks, frames=frames, tmp=tmp, shifts=tool_shifts(H, W))


def expect(prev, changes, shifts):
    """prev: a stage; changes: {field: (invalidated (N, H, W) bool, invalid)} -> the stage the model predicts"""
    st = {"planes": {k: v.copy() for k, v in prev["planes"].items()}, "dst": {}, "xyz": [x.copy() for x in prev["xyz"]]}
    for name, (inv, invalid) in changes.items():
        st["planes"][name] = M.apply(prev["planes"][name], inv, invalid)
        for k, rname in enumerate(("RANGE", "RANGE2")):
            if name == rname:
                st["xyz"][k][inv.reshape(N, H * W)] = 0.0
    for name in ("RANGE", "REFLECTIVITY"):
        st["dst"][name] = np.stack([M.destagger(st["planes"][name][f], shifts) for f in range(N)])
    return st


def check(got, want, what):
    for name in want["planes"]:
        assert same(got["planes"][name], want["planes"][name]), (what, name)
    for name in want["dst"]:
        assert same(got["dst"][name], want["dst"][name]), (what, "destaggered", name)
    for k in range(2):
        assert same(got["xyz"][k], want["xyz"][k]), (what, "xyz", k)


def test_decode_baseline_is_consistent(run):
    s0, sh = run["stages"][0], run["shifts"]
    assert {"RANGE", "RANGE2", "REFLECTIVITY", "REFLECTIVITY2", "NEAR_IR"} <= set(s0["planes"])
    for f in range(N):
        assert np.array_equal(s0["planes"]["RANGE"][f], run["frames"][f].plane("RANGE"))
    for name in ("RANGE", "REFLECTIVITY"):
        assert same(s0["dst"][name], np.stack([M.destagger(s0["planes"][name][f], sh) for f in range(N)]))
    assert not same(s0["xyz"][0][0], s0["xyz"][0][1])


def test_clip(run):
    s, p = run["stages"], run["params"]
    inv = ~M.inside(s[0]["planes"]["RANGE"], p["clip_lo"], p["clip_hi"])
    nontrivial(inv)
    check(s[1], expect(s[0], {"RANGE": (inv, 0)}, run["shifts"]), "clip")


def test_filter_field(run):
    s, p = run["stages"], run["params"]
    inv = M.key_invalidated(s[1]["planes"]["REFLECTIVITY"], p["key_lo"], p["key_hi"])
    nontrivial(inv)
    check(s[2], expect(s[1], {n: (inv, 0) for n in s[1]["planes"]}, run["shifts"]), "filter_field")


def test_filter_uv(run):
    s = run["stages"]
    inv = np.stack([M.cols_invalidated(H, W, run["shifts"], W - W // 8, W)] * N)
    assert np.array_equal(inv[0], M.cols_invalidated_via_destagger(H, W, run["shifts"], W - W // 8, W))
    nontrivial(inv)
    want = expect(s[2], {n: (inv, 0) for n in s[2]["planes"]}, run["shifts"])
    rows = np.stack([M.rows_invalidated(H, W, 1, 3)] * N)
    nontrivial(rows)
    want["planes"]["NEAR_IR"] = M.apply(want["planes"]["NEAR_IR"], rows, 5)
    check(s[3], want, "filter_uv")


def test_mask_per_sensor(run):
    s = run["stages"]
    inv = np.stack([M.mask_invalidated(run["masks"][f % 2]) for f in range(N)])
    nontrivial(inv)
    assert not np.array_equal(inv[0], inv[1])
    check(s[4], expect(s[3], {"RANGE2": (inv, 0), "REFLECTIVITY": (inv, 0)}, run["shifts"]), "mask")


def test_filter_xyz_reads_the_batchs_own_cloud(run):
    s, p = run["stages"], run["params"]
    inv = [np.stack([M.xyz_invalidated(s[4]["xyz"][k][f], 2, p["z_lo"], p["z_hi"], H, W) for f in range(N)]) for k in range(2)]
    nontrivial(inv[0])
    nontrivial(inv[1])
    changes = {n: (inv[1] if M.xyz_source(n, True, True) == "RANGE2" else inv[0], 0) for n in s[4]["planes"]}
    check(s[5], expect(s[4], changes, run["shifts"]), "filter_xyz")


def test_clouds_equal_cartesian_of_the_filtered_range_and_refusals(run):
    assert "cartesian_equal 1" in run["stdout"], run["stdout"]
    assert "refusals ok" in run["stdout"], run["stdout"]
    check(run["stages"][6], run["stages"][5], "after the refused calls")


def test_dewarp_after_range_filters_counts_again(run):
    """The decode counted the gate on the UNFILTERED ranges; dewarp(gate) must not reuse those counts."""
    s, p = run["stages"], run["params"]
    lo, hi = math.ceil(p["gate_min"] * 1e3), math.floor(p["gate_max"] * 1e3)
    pts, offs = [], [0]
    stale = 0
    for f in range(N):
        r = s[5]["planes"]["RANGE"][f]
        r0 = s[0]["planes"]["RANGE"][f]
        status = np.asarray(run["frames"][f].status)
        valid = np.nonzero(status & 1)[0]
        cols = [c for c in range(valid[0], valid[-1] + 1) if status[c] != 0]
        keep = np.zeros((H, W), bool)
        keep[:, cols] = True
        keep &= (r >= lo) & (r <= hi)
        stale += int((((r0 >= lo) & (r0 <= hi))[:, cols]).sum())
        cloud = s[5]["xyz"][0][f].reshape(H, W, 3)
        pts.append(cloud.transpose(1, 0, 2)[keep.T])   # column by column, rows top to bottom
        offs.append(offs[-1] + int(keep.sum()))
    want = np.concatenate(pts)
    assert stale > offs[-1] > 0   # the stale counts would have promised more points
    got_off = np.fromfile(run["tmp"] / "o.dwoff", np.uint64)
    assert got_off.tolist() == offs
    got = np.fromfile(run["tmp"] / "o.dw", np.float64).reshape(-1, 3)
    # identity poses: R p + t adds exact zeros; value equality (a -0.0 coordinate may come back as +0.0)
    assert got.shape == want.shape and np.array_equal(got, want)
