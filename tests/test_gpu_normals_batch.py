"""normals on a resident hip::DeviceFrameBatch, through tests/cpp/normals_batch_tool.cpp: 5 dual-return frames of the two small
sensors of the pose batch test (each with a sensor_to_body of its own), one packet of one frame left out.  Three batches -- body
frame f64, body frame float, world frame after interp_poses with 9 known poses -- and for each the downloaded normals must equal
tests/normals_model.py run on the batch's OWN downloaded clouds, ranges and poses, bit for bit: in the destaggered layout, in the
staggered one (normal i belongs to point i), for the single-return form, and again after filter_field on RANGE.  The ranges are a
smooth scene (a slanted wall with a step, a second return some hundred mm behind it), so that the model takes its cases B and C
and not only the lone-pixel case A; the model's classification is asserted.  A batch without XYZ, and the dual form on a batch
without RANGE2, throw std::invalid_argument."""
import numpy as np
import pytest

import cpp_tools
import normals_model as M
from batch_cases import FILTER_HI, FILTER_LO, H, K, N, SKIP_FRAME, SKIP_PACKET, W, scene, write_known, write_packets
from conftest import has_gpu

pytestmark = pytest.mark.gpu


def destagger(a, shifts):
    """staggered (N, H, W, ...) -> destaggered: pixel (u, v) lies at column (v - shift[u]) mod W"""
    out = np.empty_like(a)
    for u in range(H):
        out[:, u] = np.roll(a[:, u], int(shifts[u]), axis=1)
    return out


@pytest.fixture(scope="module")
def run(oracle, tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("normals_batch")
    write_packets(oracle, tmp, scene)
    write_known(tmp)
    res = cpp_tools.run("normals_batch_tool", [tmp / "packets.bin", H, W, N, SKIP_FRAME, SKIP_PACKET, tmp / "known.bin", K, tmp / "o", FILTER_LO, FILTER_HI])
    out = {"stdout": res.stdout, "s2b": np.fromfile(tmp / "o.s2b", np.float64).reshape(2, 16),
           "shifts": np.fromfile(tmp / "o.shifts", np.int32)}
    assert out["shifts"].shape == (H,) and (out["shifts"] > 0).any() and (out["shifts"] < 0).any()
    for tag, ft in (("body64", np.float64), ("body32", np.float32), ("world64", np.float64)):
        b = {}
        for pre in ("", "f") if tag == "body64" else ("",):
            for r in (0, 1):
                b[pre + "xyz%d" % r] = np.fromfile(tmp / ("o.%s.%sxyz%d" % (tag, pre, r)), ft).reshape(N, H, W, 3)
                b[pre + "r%d" % r] = np.fromfile(tmp / ("o.%s.%sr%d" % (tag, pre, r)), np.uint32).reshape(N, H, W)
        names = ["single", "d0", "d1", "s0", "s1"] + (["fd0", "fd1"] if tag == "body64" else [])
        for name in names:
            b[name] = np.fromfile(tmp / ("o.%s.%s" % (tag, name)), np.float64).reshape(N, H, W, 3)
        if tag == "world64":
            b["poses"] = np.fromfile(tmp / "o.world64.poses", np.float64).reshape(N, W, 16)
        out[tag] = b
    return out


def origins(run, tag, f):
    s2b = run["s2b"][f % 2]
    if tag == "world64":
        return M.sensor_origins(run[tag]["poses"][f], s2b)
    return np.tile(s2b.reshape(4, 4)[:3, 3], (W, 1))


def model(run, tag, pre, psr, dual=True, classify=False):
    """the model on the batch's own downloads, destaggered with the first sensor's shifts: per frame what M.normals returns"""
    b, sh = run[tag], run["shifts"]
    x0, x1 = destagger(b[pre + "xyz0"].astype(np.float64), sh), destagger(b[pre + "xyz1"].astype(np.float64), sh)
    r0, r1 = destagger(b[pre + "r0"], sh), destagger(b[pre + "r1"], sh)
    res = []
    for f in range(N):
        kw = dict(sensor_origins_xyz=origins(run, tag, f), pixel_search_range=psr, classify=classify)
        if dual:
            res.append(M.normals(x0[f].reshape(-1, 3), r0[f], x1[f].reshape(-1, 3), r1[f], **kw))
        else:
            res.append(M.normals(x0[f].reshape(-1, 3), r0[f], **kw))
    return res


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got, np.float64).view(np.uint64), np.ascontiguousarray(want, np.float64).view(np.uint64))


def test_the_batches_hold_what_the_test_encoded(run):
    b = run["body64"]
    sh = run["shifts"]
    for f in range(N):
        keep = b["r0"][f] != 0
        w1, w2 = scene(f, keep)
        assert np.array_equal(b["r0"][f], w1) and np.array_equal(b["r1"][f], w2)
        missing = np.zeros(W, bool)
        if f == SKIP_FRAME:
            missing[SKIP_PACKET * 16:(SKIP_PACKET + 1) * 16] = True
        assert not keep[:, missing].any() and 0.8 < keep[:, ~missing].mean() < 0.97
    assert np.array_equal(run["body32"]["r0"], b["r0"]) and np.array_equal(run["world64"]["r1"], b["r1"])
    # the three clouds differ as their frames do: float against double, world against body
    assert not np.array_equal(run["body32"]["xyz0"].astype(np.float64), b["xyz0"])
    assert np.abs(run["world64"]["xyz0"] - b["xyz0"]).max() > 1.0
    # the origins the batch must use are not zero, differ between the two sensors and, in the world frame, between columns
    assert np.abs(origins(run, "body64", 0)).min() > 0.1 and not np.array_equal(origins(run, "body64", 0), origins(run, "body64", 1))
    ow = origins(run, "world64", 2)
    assert len({tuple(o) for o in ow[destagger(b["r0"], sh)[2].any(axis=0)]}) > W // 2
    assert "no_xyz_throws 1" in run["stdout"] and "no_range2_throws 1" in run["stdout"]
    for tag in ("body64", "body32", "world64"):
        assert "device_ptr %s 1" % tag in run["stdout"]


def test_the_scene_takes_the_models_cases(run):
    codes = set()
    for res in model(run, "body64", "", 1, classify=True):
        codes |= set(res[2].tolist()) | set(res[3].tolist())
    assert {M.ZERO_RANGE, M.CASE_C, M.CASE_C_FLIP} <= codes and (M.CASE_B_VERTICAL in codes or M.CASE_B_HORIZONTAL in codes)
    # and the origin matters to the answer: zeros instead of the mount's translation change normals
    b, sh = run["body64"], run["shifts"]
    x0, r0 = destagger(b["xyz0"], sh)[0], destagger(b["r0"], sh)[0]
    x1, r1 = destagger(b["xyz1"], sh)[0], destagger(b["r1"], sh)[0]
    zero = M.normals(x0.reshape(-1, 3), r0, x1.reshape(-1, 3), r1, sensor_origins_xyz=np.zeros((W, 3)))
    assert not same_bits(zero[0], b["d0"][0].reshape(-1, 3))


@pytest.mark.parametrize("tag", ["body64", "body32", "world64"])
def test_destaggered_normals_equal_the_model(run, tag):
    for f, (n0, n1) in enumerate(model(run, tag, "", 1)):
        assert same_bits(run[tag]["d0"][f].reshape(-1, 3), n0), (tag, f)
        assert same_bits(run[tag]["d1"][f].reshape(-1, 3), n1), (tag, f)
    assert np.abs(run[tag]["d0"]).max() > 0.5


@pytest.mark.parametrize("tag", ["body64", "body32", "world64"])
def test_staggered_normals_belong_to_the_batchs_points(run, tag):
    sh = run["shifts"]
    got0, got1 = destagger(run[tag]["s0"], sh), destagger(run[tag]["s1"], sh)
    for f, (n0, n1) in enumerate(model(run, tag, "", 2)):
        assert same_bits(got0[f].reshape(-1, 3), n0), (tag, f)
        assert same_bits(got1[f].reshape(-1, 3), n1), (tag, f)
    # normal i belongs to point i: none where the staggered point has no range, one wherever it has
    has = np.abs(run[tag]["s0"]).sum(axis=-1) > 0
    assert not has[run[tag]["r0"] == 0].any() and has[run[tag]["r0"] != 0].mean() > 0.9


@pytest.mark.parametrize("tag", ["body64", "body32", "world64"])
def test_single_return_form(run, tag):
    for f, n0 in enumerate(model(run, tag, "", 3, dual=False)):
        assert same_bits(run[tag]["single"][f].reshape(-1, 3), n0), (tag, f)


def test_normals_again_after_filter_field_on_range(run):
    b = run["body64"]
    inside = (b["r0"] >= FILTER_LO) & (b["r0"] <= FILTER_HI)
    assert 0.05 < inside.mean() < 0.6
    assert not b["fr0"][inside].any() and np.array_equal(b["fr0"][~inside], b["r0"][~inside])
    assert not b["fxyz0"][inside].any()
    for f, (n0, n1) in enumerate(model(run, "body64", "f", 1)):
        assert same_bits(b["fd0"][f].reshape(-1, 3), n0), f
        assert same_bits(b["fd1"][f].reshape(-1, 3), n1), f
    assert not same_bits(b["fd0"], b["d0"])
