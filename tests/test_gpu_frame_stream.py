"""hip::FrameStream through tests/cpp/stream_tool.cpp: the scenarios of tests/stream_cases.py -- ring laps with different totals, one
batch in flight, f64 points, two sensors, a batch at capacity, batches without points, an empty gate, finish() midway, push_packet,
the non-compacting route, a plane list without RANGE -- each run once by a module fixture.  Every delivered batch is held

  - to the oracle (stream_cases.want): planes, destaggered planes, headers, frame_offsets, n_points and provenance bit for bit;
    points within 1e-4 m (f32) / 1e-9 m (f64), the bars of tests/test_gpu_dewarp_frames.py::FORMS (rows32, sep64); dense clouds
    within 4e-5 m (f32, tests/test_gpu_parity.py) / 1e-9 m (f64);
  - to ONE DeviceFrameBatch of all the frames with the same options: byte for byte, which is far tighter than the bars and holds
    because decode and dewarp work frame by frame -- what a batch computes for a frame does not depend on the batch around it;
  - to its bookkeeping: first_frame without gaps, frames_pushed == frames_delivered, null pointers exactly where the options say.

The frames of `laps` also go through six (frames per batch, batches in flight) pairs and must give the same bytes; the constructor
must refuse what it cannot serve.  The preconditions these tests lean on are tests/test_stream_cases_cpu.py."""
import numpy as np
import pytest

import cpp_tools
import stream_cases as S
from conftest import has_gpu

pytestmark = pytest.mark.gpu

H, W = S.H, S.W
NAMES = list(S.SCENARIOS)
PLANE_DTYPE = {"RANGE": np.uint32, "RANGE2": np.uint32, "REFLECTIVITY": np.uint8, "REFLECTIVITY2": np.uint8, "NEAR_IR": np.uint8}
PROVENANCE = ("point_frame_idxs", "point_col_idxs", "point_timestamps_ns")
FILE_OF = {"point_frame_idxs": ("frame_idxs", np.uint32), "point_col_idxs": ("col_idxs", np.uint32),
           "point_timestamps_ns": ("timestamps_ns", np.uint64), "timestamp": ("timestamp", np.uint64),
           "measurement_id": ("measurement_id", np.uint16), "status": ("status", np.uint32)}


def load(tmp, name, side):
    """everything one side ("stream" or "batch") wrote for a scenario, each array the concatenation over the batches"""
    sc = S.SCENARIOS[name]
    T = np.float64 if sc.f64 else np.float32
    pre = str(tmp / name) + "." + side + "."
    d = {"planes": {p: np.fromfile(pre + "plane." + p, PLANE_DTYPE[p]).reshape(-1, H, W) for p in sc.planes},
         "destaggered": {p: np.fromfile(pre + "dst." + p, PLANE_DTYPE[p]).reshape(-1, H, W) for p in sc.destaggered}}
    for key in ("timestamp", "measurement_id", "status"):
        d[key] = np.fromfile(pre + FILE_OF[key][0], FILE_OF[key][1]).reshape(-1, W)
    if sc.xyz:
        d["xyz"] = [np.fromfile(pre + "xyz%d" % k, T).reshape(-1, H * W, 3) for k in range(2)]
    if sc.gate is not None:
        d["offsets"] = np.fromfile(pre + "offsets", np.uint64)
        d["points"] = np.fromfile(pre + "points", T).reshape(-1, 3)
        if sc.provenance:
            for key in PROVENANCE:
                d[key] = np.fromfile(pre + FILE_OF[key][0], FILE_OF[key][1])
    return d


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("frame_stream")
    S.write_packets(oracle, tmp / "packets.bin")
    out = {"tmp": tmp}
    for name in NAMES + ["refusals"]:
        res = cpp_tools.run("stream_tool", [tmp / "packets.bin", name, tmp / name], timeout=60)
        lines = [ln.split() for ln in res.stdout.splitlines()]
        r = {"stdout": res.stdout,
             "batches": [dict(first_frame=int(ln[1]), n_frames=int(ln[2]), n_points=int(ln[3]),
                              null=set(ln[4][len("null="):].split(",")) - {""}, maps=ln[5][len("maps="):])
                         for ln in lines if ln and ln[0] == "batch"],
             "frames": [tuple(int(x) for x in ln[1:]) for ln in lines if ln and ln[0] == "frames"],
             "one_shot": [tuple(int(x) for x in ln[1:]) for ln in lines if ln and ln[0] == "one_shot"]}
        if name != "refusals":
            r["stream"], r["batch"] = load(tmp, name, "stream"), load(tmp, name, "batch")
        out[name] = r
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def global_frame_idxs(r):
    """point_frame_idxs of a stream, the index within the batch, as the index in push order"""
    add = np.concatenate([np.full(b["n_points"], b["first_frame"], np.uint32) for b in r["batches"]] + [np.zeros(0, np.uint32)])
    return r["stream"]["point_frame_idxs"] + add


def global_offsets(sc, r):
    """the batches' frame_offsets strung together: [frames + 1]; the unused frames of a partial batch must add nothing"""
    per = r["stream"]["offsets"].reshape(len(r["batches"]), sc.fpb + 1)
    out, base = [0], 0
    for b, off in zip(r["batches"], per):
        assert off[0] == 0 and (off[b["n_frames"]:] == off[b["n_frames"]]).all() and off[-1] == b["n_points"], (b, off)
        out += [base + int(x) for x in off[1:b["n_frames"] + 1]]
        base += int(off[-1])
    return np.array(out, np.uint64)


@pytest.mark.parametrize("name", NAMES)
def test_every_batch_equals_the_oracle(oracle, runs, name):
    sc, r, want = S.SCENARIOS[name], runs[name], S.want(oracle, name)
    got = r["stream"]
    assert [(b["first_frame"], b["n_frames"]) for b in r["batches"]] == [(b["first_frame"], b["n_frames"]) for b in want]
    cat = lambda key, sub=None: np.concatenate([(b[key] if sub is None else b[key][sub]) for b in want])
    for p in sc.planes:
        assert same(got["planes"][p], cat("planes", p)), p
    for p in sc.destaggered:
        assert same(got["destaggered"][p], cat("destaggered", p)), p
    for key in ("timestamp", "measurement_id", "status"):
        assert same(got[key], cat(key)), key
    worst = {}
    if sc.xyz:
        bar = S.F64_CLOUD_BAR if sc.f64 else S.F32_CLOUD_BAR
        for k in range(2):
            w = cat("xyz", k)
            assert got["xyz"][k].shape == w.shape and got["xyz"][k].dtype == w.dtype
            worst["cloud %d" % k] = (float(np.abs(got["xyz"][k].astype(np.float64) - w.astype(np.float64)).max()), bar)
    if sc.gate is not None:
        assert [b["n_points"] for b in r["batches"]] == [b["n_points"] for b in want]
        assert same(got["offsets"], cat("frame_offsets"))
        w = cat("points")
        assert got["points"].shape == w.shape and got["points"].dtype == w.dtype
        bar = S.F64_POINT_BAR if sc.f64 else S.F32_POINT_BAR
        worst["points"] = (float(np.abs(got["points"].astype(np.float64) - w.astype(np.float64)).max()) if len(w) else 0.0, bar)
        if sc.provenance:
            for key in PROVENANCE:
                assert same(got[key], cat(key)), key
    print("%s: largest error %s" % (name, ", ".join("%s %.3g m (bar %g)" % (k, v[0], v[1]) for k, v in worst.items()) or "none to measure"))
    for what, (err, bar) in worst.items():
        assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("name", NAMES)
def test_the_stream_equals_one_batch_of_all_frames(runs, name):
    sc, r = S.SCENARIOS[name], runs[name]
    got, one = r["stream"], r["batch"]
    n = sum(b["n_frames"] for b in r["batches"])
    assert r["one_shot"] == [(n, sum(b["n_points"] for b in r["batches"]))]
    for p in sc.planes:
        assert same(got["planes"][p], one["planes"][p]), p
    for p in sc.destaggered:
        assert same(got["destaggered"][p], one["destaggered"][p]), p
    for key in ("timestamp", "measurement_id", "status"):
        assert same(got[key], one[key]), key
    if sc.xyz:
        for k in range(2):
            assert same(got["xyz"][k], one["xyz"][k]), k
    if sc.gate is not None:
        assert same(global_offsets(sc, r), one["offsets"])
        assert same(got["points"], one["points"])
        if sc.provenance:
            assert same(global_frame_idxs(r), one["point_frame_idxs"])
            assert same(got["point_col_idxs"], one["point_col_idxs"])
            assert same(got["point_timestamps_ns"], one["point_timestamps_ns"])


@pytest.mark.parametrize("name", NAMES)
def test_bookkeeping_and_null_pointers(oracle, runs, name):
    sc, r = S.SCENARIOS[name], runs[name]
    released = len(S.decoded_frames(oracle, sc))
    at = 0
    for b in r["batches"]:      # push order, no gaps
        assert b["first_frame"] == at and 1 <= b["n_frames"] <= sc.fpb
        at += b["n_frames"]
    assert at == released and r["frames"] == [(released, released)]
    null = set()
    if not sc.xyz:
        null |= {"xyz0", "xyz1"}
    if sc.gate is None:
        null |= {"points", "frame_offsets"}
    if sc.gate is None or not sc.provenance:
        null |= set(PROVENANCE)
    maps = ",".join(sorted(sc.planes)) + ("," if sc.planes else "") + "|" + ",".join(sorted(sc.destaggered)) + ("," if sc.destaggered else "")
    for b in r["batches"]:
        assert b["null"] == null, (b, null)
        assert b["maps"] == maps, (b, maps)
        if sc.gate is None:
            assert b["n_points"] == 0


def test_the_frames_of_laps_give_the_same_bytes_however_they_are_batched(runs):
    base = runs["laps"]
    keys = ("points", "point_col_idxs", "point_timestamps_ns")
    for fpb, in_flight in S.INVARIANCE:
        name = "laps_%dx%d" % (fpb, in_flight)
        r = runs[name]
        assert len(r["batches"]) == -(-11 // fpb), name
        for key in keys:
            assert same(r["stream"][key], base["stream"][key]), (name, key)
        assert same(global_frame_idxs(r), global_frame_idxs(base)), name
        assert same(global_offsets(S.SCENARIOS[name], r), global_offsets(S.SCENARIOS["laps"], base)), name
        assert same(r["stream"]["planes"]["RANGE"], base["stream"]["planes"]["RANGE"]), name
    assert len(base["stream"]["points"]) > 1000
    assert [b["n_frames"] for b in runs["laps_16x2"]["batches"]] == [11]      # one partial batch


def test_a_plane_list_without_range_gets_it_added(runs):
    a, b = runs["range_added"], runs["laps"]
    assert len(a["stream"]["points"]) > 1000
    for key in ("points", "offsets") + PROVENANCE:
        assert same(a["stream"][key], b["stream"][key]), key
    assert a["batches"][0]["maps"] == "REFLECTIVITY,|"       # what the caller asked to download, no more


def test_the_constructor_refuses_what_it_cannot_serve(runs):
    lines = [ln for ln in runs["refusals"]["stdout"].splitlines() if ln.startswith("refusal ")]
    assert [ln.split()[1] for ln in lines] == ["download_of_a_plane_not_kept", "download_of_a_destaggered_only_plane", "no_sensors",
                                               "frames_per_batch_not_a_multiple", "no_batches_in_flight"], runs["refusals"]["stdout"]
    assert all(ln.split()[2] == "1" for ln in lines), runs["refusals"]["stdout"]
