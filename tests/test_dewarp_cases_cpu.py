"""CPU: the batches of tests/dewarp_cases.py are what tests/test_gpu_dewarp_frames.py needs them to be -- asserted from the
oracle alone, so that a GPU test that passes has passed on an input that could have failed."""
import numpy as np
import pytest

import dewarp_cases as D


def _frame_cols(c, O, gate, f):
    return c.want(O, gate, np.float64)["per_frame"][f][1]


def test_raw_gates():
    """the gates of the GPU tests in millimetres (the GPU tests assert that ouster_hip_range_gate gives the same)"""
    assert D.raw_gate(1.0, 60.0) == (1000, 60000) and D.raw_gate(0.0, 1000.0) == (0, 1000000) and D.raw_gate(2.0, 90.0) == (2000, 90000)
    assert D.IN_GATE in range(1000, 60001)


@pytest.mark.parametrize("gate", D.GATES)
@pytest.mark.parametrize("h,w,n", D.WIDE_SHAPES)
def test_wide_frames(oracle, h, w, n, gate):
    c = D.wide(h, w, n)
    f = c.facts
    st, kept = c.status, c.kept(gate)
    cols0 = _frame_cols(c, oracle, gate, 0)
    # frame 0 keeps points in every block of 2048 columns, and its span is first..last
    blocks = (w + D.SCAN_BLOCK - 1) // D.SCAN_BLOCK
    assert set((cols0 // D.SCAN_BLOCK).tolist()) == set(range(blocks))
    assert cols0.min() >= f["first"] and cols0.max() <= f["last"]
    valid = np.flatnonzero(st[0] & 1)
    assert valid.min() == f["first"] and valid.max() == f["last"]
    assert st[0, 2047] == 0 and 2047 not in cols0 and kept[0, :, 2047].any()
    if w > 2048:
        assert st[0, 2048] != 0 and st[0, 2048] != 1 and 2048 in cols0
    # the status-2 columns outside the span hold in-gate ranges: emitting them would show
    assert len(f["outside"]) == (2 if w == 2049 else 4)
    for x in f["outside"]:
        assert st[0, x] == 2 and kept[0, :, x].any() and x not in cols0 and (x < f["first"] or x > f["last"])
    others = np.setdiff1d(np.concatenate([np.arange(f["first"]), np.arange(f["last"] + 1, w)]), f["outside"])
    assert not st[0, others].any()
    # frame 1: nothing valid below lo1 (a later block where the frame has one), and not empty
    cols1 = _frame_cols(c, oracle, gate, 1)
    assert not st[1, :f["lo1"]].any() and len(cols1) > 0 and cols1.min() >= f["lo1"]
    assert f["lo1"] == (2048 if w > 2048 else w - 8)
    if n > 2:
        cols2 = _frame_cols(c, oracle, gate, 2)
        assert len(cols2) > 0 and set(cols2.tolist()) == {w - 1}
    # the synthetic gate counts are the true counts, and use some slots never
    gc = c.synthetic_gate_counts(gate)
    assert gc.shape == (n, 8, w) and not gc[:, [1, 4, 6]].any() and gc.any()


@pytest.mark.parametrize("n,empty_256", [(256, False), (257, False), (520, False), (257, True), (520, True)])
def test_long_batches(oracle, n, empty_256):
    c = D.long_batch(n, empty_256)
    gate = D.GATES[0]
    w64, w32 = c.want(oracle, gate, np.float64), c.want(oracle, gate, np.float32)
    per = np.diff(w64["frame_offsets"].astype(np.int64))
    assert np.array_equal(w64["frame_offsets"], w32["frame_offsets"])
    for f in D.NON_EMPTY:
        if f < n and not (empty_256 and f == 256):
            assert per[f] > 0, f
    if empty_256:
        assert per[256] == 0 and per[255] > 0
    assert all(m % 3 for m in D.LONG_N)          # no size is a multiple of the three LUTs
    seventh = np.arange(n) % 7 == 6
    assert not per[seventh].any() and (per[~seventh] > 0).sum() >= (~seventh).sum() - 1
    # a kernel that ignored f % n_luts would fail: the twins differ only by their LUT
    a, b = D.TWIN
    assert a % 3 != b % 3 and np.array_equal(c.r[a], c.r[b]) and np.array_equal(c.status[a], c.status[b])
    pa, pb = w32["per_frame"][a][0], w32["per_frame"][b][0]
    assert pa.shape == pb.shape and len(pa) > 0 and np.abs(pa.astype(np.float64) - pb).min() > 1e-2


@pytest.mark.parametrize("n,n_luts", [(7, 3), (5, 2)])
def test_multi_lut_batches(oracle, n, n_luts):
    c = D.multi_lut(n, n_luts)
    for gate in D.GATES:
        w = c.want(oracle, gate, np.float64)
        assert (np.diff(w["frame_offsets"].astype(np.int64)) > 0).all()
    luts = [c.lut_arrays(oracle, k, np.float64) for k in range(n_luts)]
    for k in range(1, n_luts):
        # directions are per millimetre of range (|d| = 1e-3), offsets in metres
        assert np.abs(luts[k][0] - luts[0][0]).max() > 1e-3 and np.abs(luts[k][1] - luts[0][1]).max() > 0.1


@pytest.mark.parametrize("gate", D.GATES)
@pytest.mark.parametrize("h,w,n", D.CAP_SHAPES)
def test_capacity_cuts(oracle, h, w, n, gate):
    c = D.capacity(h, w, n)
    want = c.want(oracle, gate, np.float64)
    offs, col0 = want["frame_offsets"].astype(np.int64), want["per_frame"][0][1]
    tot = int(offs[-1])
    assert tot > 64
    caps = D.capacities(c, oracle, gate)
    flat_cols = want["col_idxs"]
    # the run that is cut has at least 3 points and the cut lies strictly inside it
    cut = caps["inside_run"]
    assert (col0 == D.CUT_COL).sum() >= 3
    assert flat_cols[cut - 1] == D.CUT_COL and flat_cols[cut] == D.CUT_COL and cut < offs[1]
    for label, x in (("column_start", D.START_COL), ("tile_start", 64)):
        k = caps[label]
        assert 0 < k < offs[1] and flat_cols[k] == x and flat_cols[k - 1] < x, label
    assert caps["frame_start"] == offs[1] and 0 < offs[1] < tot
    if n > 2:
        assert offs[1] == offs[2] and not (c.status[1] & 1).any()      # the frame without valid columns
    if h > 128:
        # some column keeps a point in rows 128-129 after keeping at least one in rows 0-127, and the cut lies between the
        # two points the second chunk writes
        kept = c.kept(gate)[0, :, D.CHUNK_COL]
        k1, k2 = int(kept[:128].sum()), int(kept[128:].sum())
        s = c.column_start(oracle, gate, 0, D.CHUNK_COL)
        assert k1 >= 1 and k2 == 2 and caps["chunk2"] == s + k1 + 1
        assert flat_cols[caps["chunk2"] - 1] == D.CHUNK_COL and flat_cols[caps["chunk2"]] == D.CHUNK_COL
    else:
        assert "chunk2" not in caps
    assert len(set(caps.values())) == len(caps) and max(caps.values()) == tot + 5 <= n * h * w


@pytest.mark.parametrize("h,w,n", D.ALIGN_SHAPES)
def test_alignment_batches(oracle, h, w, n):
    c = D.alignment(h, w, n)
    assert w % 4 == 0           # the vector staging is what an aligned call of these shapes takes
    for gate in D.GATES:
        assert (np.diff(c.want(oracle, gate, np.float64)["frame_offsets"].astype(np.int64)) > 0).all()
