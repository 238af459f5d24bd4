"""Inputs the tests of the range-gated frame dewarp share (tests/test_dewarp_cases_cpu.py, test_gpu_dewarp_frames.py): no test
in here.  A Case holds a batch of frames built like test_gpu_parity.py::test_dewarp_frames_matches_oracle builds its own
(synthetic_calib(h, w, b2l_x=15.806), ranges below 2^17 with about 30 % zeros, per-column yaw poses with translations within
+-20 m, random 62-bit timestamps), the oracle's answer per gate and type (oracle.dewarp_frame, LUT f % n_luts for frame f) and
the facts a test relies on.  The builders below give the batches of the five sections of test_gpu_dewarp_frames.py."""
import math

import numpy as np

GATES = ((1.0, 60.0), (0.0, 1000.0))
SCAN_BLOCK = 2048      # columns k_dwf_scan takes per pass (k_dewarp.hip: 256 threads x 8)
FRAME_BLOCK = 256      # frame totals k_dwf_frame_scan takes per pass
GATE_CHUNKS = 8        # OUSTER_HIP_GATE_CHUNKS: partial counts per column in gate_counts[f][8][W]
IN_GATE = 5000         # a range inside both gates


def raw_gate(lo, hi):
    """(min_r, max_r) of a gate in metres that is neither empty nor saturated: ceil / floor of the millimetres
    (impl/dewarp_impl.h:33-34; tests/test_range_gate_cpu.py has the edges)."""
    return int(math.ceil(lo * 1e3)), int(math.floor(hi * 1e3))


def extrinsic(k):
    """LUT k of a batch with several: a rotation about z by 90 degrees * k and an own translation, so that the same range
    image gives visibly different points."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
    ext = np.eye(4)
    ext[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    ext[:3, 3] = [1.5 * k, -2.0 + k, 0.25 * k]
    return ext


class Case:
    def __init__(self, name, h, w, n, n_luts=1, seed=None):
        self.name, self.h, self.w, self.n, self.n_luts = name, h, w, n, n_luts
        g = np.random.default_rng(h * 31 + w + 7919 * n if seed is None else seed)
        r = g.integers(0, 2 ** 17, size=(n, h, w)).astype(np.uint32)
        r[g.random(r.shape) < 0.3] = 0
        self.r = r
        self.status = np.ones((n, w), dtype=np.uint32)
        self.ts = g.integers(1, 2 ** 62, size=(n, w)).astype(np.uint64)
        poses = np.tile(np.eye(4), (n, w, 1, 1))
        ang = g.uniform(-0.3, 0.3, size=(n, w))
        poses[..., 0, 0] = np.cos(ang); poses[..., 0, 1] = -np.sin(ang)
        poses[..., 1, 0] = np.sin(ang); poses[..., 1, 1] = np.cos(ang)
        poses[..., :3, 3] = g.uniform(-20, 20, size=(n, w, 3))
        self.poses = poses
        self.facts = {}
        self._want, self._cals = {}, None

    def freeze(self):
        for a in (self.r, self.status, self.ts, self.poses):
            a.setflags(write=False)
        return self

    # -- the LUTs ------------------------------------------------------------------------------------------------------
    def cals(self, O):
        if self._cals is None:
            self._cals = []
            for k in range(self.n_luts):
                cal = O.synthetic_calib(h=self.h, w=self.w, b2l_x=15.806)
                if self.n_luts > 1:
                    cal.extrinsic = extrinsic(k)
                self._cals.append(cal)
        return self._cals

    def lut_arrays(self, O, k, T):
        d, o = self.cals(O)[k].xyz_lut(True)
        return d.astype(T), o.astype(T)

    # -- the oracle's answer ---------------------------------------------------------------------------------------------
    def want(self, O, gate, T):
        """{"frame_offsets" [n + 1] u64, "points" [tot, 3] T, "col_idxs", "frame_idxs" [tot] u32, "timestamps_ns" [tot] u64,
        "per_frame": the oracle's (points, col_idxs, timestamps) of every frame}; computed once, never written."""
        key = (tuple(gate), np.dtype(T).name)
        if key not in self._want:
            luts = [self.lut_arrays(O, k, T) for k in range(self.n_luts)]
            per = [O.dewarp_frame(self.r[f], self.status[f], self.ts[f], self.poses[f], *luts[f % self.n_luts], *gate)
                   for f in range(self.n)]
            res = {"frame_offsets": np.concatenate([[0], np.cumsum([len(x[0]) for x in per])]).astype(np.uint64),
                   "points": np.concatenate([x[0] for x in per]),
                   "col_idxs": np.concatenate([x[1] for x in per]),
                   "frame_idxs": np.concatenate([np.full(len(x[0]), f, np.uint32) for f, x in enumerate(per)]),
                   "timestamps_ns": np.concatenate([x[2] for x in per]),
                   "per_frame": per}
            for v in res.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._want[key] = res
        return self._want[key]

    def column_start(self, O, gate, f, x):
        """index, in the whole output, of the first point of column x of frame f (of the next emitted column if x emits none)"""
        w = self.want(O, gate, np.float64)
        return int(w["frame_offsets"][f]) + int(np.searchsorted(w["per_frame"][f][1], x))

    # -- gate counts ----------------------------------------------------------------------------------------------------
    def kept(self, gate):
        lo, hi = raw_gate(*gate)
        return (self.r >= lo) & (self.r <= hi)

    def true_counts(self, gate):
        """[n, w]: pixels of every column inside the gate, whatever its status (what k_dwf_count computes)"""
        return self.kept(gate).sum(axis=1).astype(np.uint32)

    def synthetic_gate_counts(self, gate, seed=11):
        """[n, 8, w] u16: the true counts split at random over the slots 0, 2, 3, 5 and 7; slots 1, 4 and 6 stay zero, and with
        few rows so do most of the others."""
        g = np.random.default_rng(seed)
        slot = g.choice(np.array([0, 2, 3, 5, 7]), size=self.r.shape)
        k = self.kept(gate)
        gc = np.stack([(k & (slot == s)).sum(axis=1) for s in range(GATE_CHUNKS)], axis=1).astype(np.uint16)
        assert np.array_equal(gc.sum(axis=1, dtype=np.uint32), self.true_counts(gate))
        return gc


# ----------------------------------------------------------------------------------------------------------------------
# A. wide frames: k_dwf_scan past one block of 2048 columns
# ----------------------------------------------------------------------------------------------------------------------
WIDE_SHAPES = [(4, 2048, 2), (4, 2052, 2), (3, 2049, 2), (8, 4096, 2), (4, 4100, 3)]


def wide(h, w, n):
    """Frame 0: valid from column 5 into the last block; status 0 at 2047 and a hole at 100, status 2 (emitted: inside the span)
    at 2048; status 2 on the two columns before the first and the two after the last valid one, 0 on everything else outside.
    Frame 1: valid columns only from 2048 on.  Frame 2: only column w - 1.
    Two shapes cannot be as the others: with w = 2048 there is no column 2048, so frame 0 ends at 2044 (2045 and 2046 carry the 2,
    2047 the 0) and frame 1 is valid in the last 8 columns; with w = 2049 column 2048 is the whole second block, so it is the
    last valid column itself, with status 3 (bit 0 set and not 1), and no column follows it."""
    c = Case(f"wide-{h}x{w}x{n}", h, w, n)
    st = c.status
    first = 5
    last = {2048: w - 4, 2049: w - 1}.get(w, w - 3)
    st[0] = 0
    st[0, first:last + 1] = 1
    st[0, 100] = 0
    st[0, 2047] = 0
    if w > 2048:
        st[0, 2048] = 3 if w == 2049 else 2
    outside = [first - 2, first - 1] + [x for x in (last + 1, last + 2) if x < w and not (w == 2048 and x == 2047)]
    st[0, outside] = 2
    lo1 = 2048 if w > 2048 else w - 8
    st[1] = 0
    st[1, lo1:] = 1
    if w - lo1 > 4:
        st[1, lo1 + 1] = 0
        st[1, lo1 + 2] = 2
    if n > 2:
        st[2] = 0
        st[2, w - 1] = 1
    # what must show if it went wrong holds in-gate ranges
    for x in outside + [2047, 100]:
        c.r[0, 0, x] = IN_GATE
    for x in (2048, w - 1, lo1):
        c.r[:, h - 1, min(x, w - 1)] = IN_GATE
    c.facts = {"first": first, "last": last, "outside": outside, "lo1": lo1}
    return c.freeze()


# ----------------------------------------------------------------------------------------------------------------------
# B. long batches: k_dwf_frame_scan past one block of 256 frames; more than one LUT
# ----------------------------------------------------------------------------------------------------------------------
LONG_N = (256, 257, 520)
NON_EMPTY = (255, 256, 257, 511, 512)
TWIN = (3, 4)    # two frames of different residue mod 3 with the same ranges, status, poses and timestamps


def long_batch(n, empty_256=False, h=4, w=16, n_luts=3):
    """n frames of 4 x 16 with three LUTs of different extrinsics.  Frames with f % 7 == 6 have all status 0 (none of 255, 256,
    257, 511, 512 is one of them: those must not be empty); the others have a few columns of status 0 and 2.  empty_256: frame
    256 itself has all status 0.  Frame 4 is a copy of frame 3."""
    c = Case(f"long-{n}" + ("-empty256" if empty_256 else ""), h, w, n, n_luts=n_luts, seed=1000 + n)
    g = np.random.default_rng(n)
    c.status[:] = g.choice(np.array([0, 1, 1, 1, 1, 1, 2, 3], np.uint32), size=(n, w))
    c.status[:, 1] = 1
    c.r[:, 0, 1] = IN_GATE              # every frame that has a valid column keeps a point
    c.status[np.arange(n) % 7 == 6] = 0
    if empty_256:
        c.status[256] = 0
    a, b = TWIN
    for arr in (c.r, c.status, c.ts, c.poses):
        arr[b] = arr[a]
    return c.freeze()


def multi_lut(n, n_luts, h=9, w=100):
    c = Case(f"luts-{n}of{h}x{w}-{n_luts}", h, w, n, n_luts=n_luts)
    c.status[0, :5] = 0
    c.status[0, w - 3:] = 0
    c.status[0, w // 2] = 0
    c.status[0, w // 2 + 1] = 2
    c.status[n - 1, ::3] = 0
    return c.freeze()


# ----------------------------------------------------------------------------------------------------------------------
# C. capacity, D. alignment
# ----------------------------------------------------------------------------------------------------------------------
CAP_SHAPES = [(130, 72, 3), (64, 128, 2)]
CUT_COL, CHUNK_COL, START_COL = 10, 11, 20   # columns of frame 0 whose runs the capacities cut


def capacity(h, w, n):
    """(130, 72, 3): two row chunks (128 + 2) and two emit tiles (64 + 8 columns); frame 1 has no valid column.  (64, 128, 2): one
    chunk, two full tiles.  Column CHUNK_COL of frame 0 keeps a point in row 0 and both rows of the second chunk."""
    c = Case(f"cap-{h}x{w}x{n}", h, w, n)
    c.status[0, :3] = 0
    c.status[0, w - 2:] = 0
    c.status[0, 30] = 0
    c.status[0, 31] = 2
    if n > 2:
        c.status[1] = 0
        c.status[1, 7] = 2
    for x in (CUT_COL, CHUNK_COL, START_COL, 64):
        c.r[0, :3, x] = IN_GATE
    if h > 128:
        c.r[0, 128:, CHUNK_COL] = IN_GATE
    return c.freeze()


def capacities(c, O, gate):
    """{label: capacity} from the oracle's offsets; "chunk2" only where the frame has a second row chunk."""
    w = c.want(O, gate, np.float64)
    tot = int(w["frame_offsets"][-1])
    col0 = w["per_frame"][0][1]
    s_cut, n_cut = c.column_start(O, gate, 0, CUT_COL), int((col0 == CUT_COL).sum())
    caps = {"zero": 0, "one": 1, "inside_run": s_cut + n_cut // 2, "column_start": c.column_start(O, gate, 0, START_COL),
            "tile_start": c.column_start(O, gate, 0, 64), "frame_start": int(w["frame_offsets"][1]),
            "tot-1": tot - 1, "tot": tot, "tot+5": tot + 5}
    if c.h > 128:
        k1 = int(c.kept(gate)[0, :128, CHUNK_COL].sum())
        caps["chunk2"] = c.column_start(O, gate, 0, CHUNK_COL) + k1 + 1
    return caps


ALIGN_SHAPES = [(7, 36, 3), (130, 72, 2)]


def alignment(h, w, n):
    c = Case(f"align-{h}x{w}x{n}", h, w, n)
    c.status[0, :2] = 0
    c.status[0, w // 2] = 0
    c.status[0, w // 2 + 1] = 2
    c.status[n - 1, w - 1] = 0
    return c.freeze()
