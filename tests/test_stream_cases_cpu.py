"""What tests/test_gpu_frame_stream.py relies on, shown without a GPU from stream_cases.want alone: the scenarios of
tests/stream_cases.py really lap the ring with different totals, reach the capacity, keep nothing, tell the two sensors apart and
lose the packets they say they lose.  A case that fails here gets other inputs, never a weaker precondition."""
import itertools

import numpy as np

import stream_cases as S


def totals(batches):
    return [b["n_points"] for b in batches]


def test_laps_uses_every_buffer_set_three_times_with_different_totals(oracle):
    sc, batches = S.SCENARIOS["laps"], S.want(oracle, "laps")
    assert [(b["first_frame"], b["n_frames"]) for b in batches] == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 2), (10, 1)]
    tot = totals(batches)
    steps = []
    for slot in range(sc.in_flight):
        uses = tot[slot::sc.in_flight]
        assert len(uses) == 3
        assert all(a != b for a, b in itertools.combinations(uses, 2)), (slot, uses)
        steps += list(zip(uses, uses[1:]))
    assert any(b < a for a, b in steps) and 0 in tot, tot
    assert any(a > 0 and b == 0 for a, b in steps), tot      # a set that held points comes back empty
    assert max(tot) > sc.fpb * S.H * S.W // 2, tot


def test_dense_frames_keep_more_than_half_of_their_pixels(oracle):
    b = S.want(oracle, "f64_three")     # one frame per batch
    for f, (kind, _) in enumerate(S.KINDS[:len(b)]):
        if kind in ("dense", "full") and f != S.MISSING_FRAME:
            assert b[f]["n_points"] > S.H * S.W // 2, f
        if kind == "far":
            assert b[f]["n_points"] == 0, f
        if kind == "full":
            assert b[f]["n_points"] == S.H * S.W and (b[f]["xyz"][0] != 0).any(axis=1).all()


def test_at_capacity_has_a_batch_exactly_at_capacity(oracle):
    sc, batches = S.SCENARIOS["at_capacity"], S.want(oracle, "at_capacity")
    cap = sc.fpb * S.H * S.W
    full = [b for b in batches if b["n_points"] == cap]
    assert full and any(b["first_frame"] == 2 for b in full)      # the two all-ranged, all-valid frames
    assert any(b["n_points"] < cap for b in batches)
    assert all(b["n_points"] <= cap for b in batches)
    # zero-range pixels of valid columns are inside this gate: the oracle counts them, and gives them the point (0, 0, 0)
    b0 = batches[0]
    assert b0["n_points"] == cap and (b0["points"] == 0).all(axis=1).sum() > 100


def test_nothing_kept_and_empty_gate_keep_nothing_of_frames_that_have_points(oracle):
    O = oracle
    for name in ("nothing_kept", "empty_gate"):
        sc, batches = S.SCENARIOS[name], S.want(O, name)
        assert batches and all(b["n_points"] == 0 and not b["frame_offsets"].any() for b in batches), name
        assert all(len(b["frame_offsets"]) == sc.fpb + 1 and len(b["points"]) == 0 for b in batches)
        under_g = sum(len(S.frame_points(O, sc, s, fr, gate=S.G)[0]) for s, fr in S.decoded_frames(O, sc))
        assert under_g > 1000, (name, under_g)


def test_two_sensors_differ_far_beyond_the_bar(oracle):
    O = oracle
    sc = S.SCENARIOS["two_sensors"]
    frames = S.decoded_frames(O, sc)
    assert [s for s, _ in frames] == [0, 1] * 5
    seen = 0
    for i, (s, fr) in enumerate(frames):
        if S.KINDS[i // 2][0] == "far":
            continue
        own = S.frame_points(O, sc, s, fr)[0].astype(np.float64)
        swapped = S.frame_points(O, sc, s, fr, lut_of=1 - s)[0].astype(np.float64)     # the wrong sensor's LUT, on purpose
        assert own.shape == swapped.shape and len(own) > S.H * S.W // 2 - (S.H * S.CPP if i // 2 == S.MISSING_FRAME else 0)
        far_apart = np.abs(own - swapped).max(axis=1) > 100 * S.F32_POINT_BAR
        assert far_apart.mean() > 0.5, (i, far_apart.mean())
        seen += 1
    assert seen == 10
    batches = S.want(O, "two_sensors")
    assert [(b["first_frame"], b["n_frames"]) for b in batches] == [(0, 4), (4, 4), (8, 2)]
    assert (batches[-1]["frame_offsets"][2:] == batches[-1]["n_points"]).all()      # the two unused frames add nothing


def test_the_frame_missing_a_packet(oracle):
    b = S.want(oracle, "laps_1x1")      # one frame per batch
    cols = np.nonzero(b[S.MISSING_FRAME]["status"][0] == 0)[0]
    assert cols.tolist() == list(range(S.MISSING_PACKET * S.CPP, (S.MISSING_PACKET + 1) * S.CPP))      # exactly 16
    assert not b[S.MISSING_FRAME]["planes"]["RANGE"][0][:, cols].any()
    assert (b[S.MISSING_FRAME - 1]["status"] == 1).all() and (b[S.MISSING_FRAME + 1]["status"] == 1).all()
    assert 0 < b[S.MISSING_FRAME]["n_points"] < b[S.MISSING_FRAME - 1]["n_points"]
    assert not (set(b[S.MISSING_FRAME]["point_col_idxs"].tolist()) & set(cols.tolist()))


def test_packets_releases_five_frames(oracle):
    O = oracle
    sc = S.SCENARIOS["packets"]
    frames = S.decoded_frames(O, sc)
    assert len(frames) == 5 and len(S.packet_sequence(O, sc)) == 6 * S.PPF - 2
    assert [(b["first_frame"], b["n_frames"]) for b in S.want(O, "packets")] == [(0, 2), (2, 2), (4, 1)]
    assert (frames[0][1]["status"] == 1).all() and (frames[1][1]["status"] == 1).all()      # the swapped packets found their frames
    lost = np.nonzero(frames[S.LOST_FRAME][1]["status"] == 0)[0]
    assert lost.tolist() == list(range(S.LOST_PACKET * S.CPP, (S.LOST_PACKET + 1) * S.CPP))
    for f in range(5):
        assert (frames[f][1]["timestamp"][:S.CPP] == S.T0_NS + f * S.FRAME_NS + np.arange(S.CPP) * S.COL_NS).all()


def test_finish_midway_spans(oracle):
    batches = S.want(oracle, "finish_midway")
    assert [(b["first_frame"], b["n_frames"]) for b in batches] == [(0, 3), (3, 4), (7, 2)]


def test_range_added_expects_what_laps_expects(oracle):
    a, b = S.want(oracle, "laps"), S.want(oracle, "range_added")
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for key in ("first_frame", "n_frames", "n_points"):
            assert x[key] == y[key]
        for key in ("frame_offsets", "points", "point_col_idxs", "point_timestamps_ns", "point_frame_idxs"):
            assert x[key].dtype == y[key].dtype and x[key].tobytes() == y[key].tobytes(), key
    assert sum(x["n_points"] for x in a) > 1000


def test_invariance_scenarios_share_the_frames_of_laps(oracle):
    base = np.concatenate([b["points"] for b in S.want(oracle, "laps")])
    for fpb, in_flight in S.INVARIANCE:
        name = "laps_%dx%d" % (fpb, in_flight)
        batches = S.want(oracle, name)
        assert np.concatenate([b["points"] for b in batches]).tobytes() == base.tobytes(), name
        assert sum(b["n_frames"] for b in batches) == 11 and all(len(b["frame_offsets"]) == fpb + 1 for b in batches)
    assert len(S.want(oracle, "laps_16x2")) == 1      # one partial batch
