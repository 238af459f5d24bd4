"""CPU-only: the tile ring of the persistent decode kernel (k_decode_stream2) as plan_stream lays it out, and its loader schedule.

tests/cpp/ring_tool.cpp -- g++ only -- prints plan_stream's StreamArgs for one PlanInput per line.  The geometries are those of the
five static profiles in tests/golden/decode_plans.json, resized to W x H.  The schedule itself (request / wait / barrier order of
a loader wave against the decoding waves) is replayed in plain Python from the plan's numbers."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp", "_build", "ring_tool")
TABLE = os.path.join(ROOT, "tests", "golden", "decode_plans.json")
LDS = 160 * 1024
WS, HS, TWS = (128, 256, 2048), (16, 32, 64, 128), (128, 256)
SPECS = {1: "dual_lb", 2: "lb", 3: "single", 4: "dual", 5: "legacy"}
TWELVE = (3, 5)   # SpecSingle, SpecLegacy: 12 B/px


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


def _tool():
    """tests/cpp/_build/ring_tool, compiled here with plan_tool's flags (g++ only: no HIP header, no library) whenever a source
    is newer than it"""
    cpp, csrc = os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "ouster_sdk_amd", "csrc")
    deps = [os.path.join(cpp, "ring_tool.cpp"), os.path.join(cpp, "plan_tool.cpp"), os.path.join(csrc, "decode_plan.cpp"),
            os.path.join(csrc, "decode_plan.h"), os.path.join(ROOT, "include", "ouster_hip.h")]
    if not os.path.exists(TOOL) or os.path.getmtime(TOOL) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", TOOL, deps[0], deps[2]])
    return TOOL


def _plans(lines):
    r = subprocess.run([_tool()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(got) == len(lines)
    return got


def _geometry(table, spec, W, H):
    cols = table["columns"]
    gi = min(dict(zip(cols, r))["geometry"] for r in table["rows"] if dict(zip(cols, r))["spec"] == spec)
    g = dict(table["geometries"][gi])
    g["pixels_per_column"], g["columns_per_frame"] = H, W
    g["col_size"] = g["col_header_size"] + H * g["channel_data_size"] + g["col_footer_size"]
    g["lidar_packet_size"] = g["packet_header_size"] + g["columns_per_packet"] * g["col_size"] + g["packet_footer_size"]
    if spec == 5:   # LEGACY: the status word sits behind the pixels
        g["col_status"] = [g["col_status"][0], g["col_header_size"] + H * g["channel_data_size"], g["col_status"][2]]
    return g


def _line(table, spec, W, H, tw, knobs=(), frames=256, xyzm=1, dst=3, host_ts=0, gate=0):
    g = _geometry(table, spec, W, H)
    stride = (g["lidar_packet_size"] + 15) // 16 * 16 + 16
    tok = [f"g.{k}={v if not isinstance(v, list) else ','.join(map(str, v))}" for k, v in g.items()]
    kn = dict(table["knob_base"], **dict(knobs))
    tok += [f"k.{k}={v}" for k, v in kn.items()]
    tok += [f"n_frames={frames}", f"slots_per_frame={W // g['columns_per_packet']}", f"packet_stride={stride}", "packets=4096", "poses=0",
            f"spec={spec}", f"xyzm={xyzm}", "vec_ok=1", "n_fields=4", "plane_mask=15", f"destagger_mask={dst}", f"xyz_mask={1 if xyzm else 0}",
            f"gate={gate}", "may_resolve=0", "cus=256", "resident_wgs=512", f"tw={tw}", f"host_ts={host_ts}"]
    return " ".join(tok)


def _grid():
    return [(s, W, H, tw) for s in SPECS for W in WS for H in HS for tw in TWS if W % tw == 0]


def _dma_per_wave(p, tw, host_ts, dst, xyzm):
    """The loader waves' instructions per tile, dealt as the kernel deals them: pixel instruction k to wave k % loader, then the
    small tables' instructions, counted from 0 again, likewise."""
    nl = p["loader"]
    small = p["n_hdr"] * (tw // 64) + p["n_pkt"] + (2 if host_ts else 0) + (-(-p["tr"] // 64) if dst else 0) + \
        (-(-p["tr"] * 18 // 64) if xyzm in (1, 2) else 0)
    per = [0, 0, 0, 0]
    for k in range(p["npix_instr"]):
        per[k % nl] += 1
    for k in range(small):
        per[k % nl] += 1
    return per


def _check_layout(p, tw):
    assert p["lds_bytes"] <= LDS
    assert 2 <= p["nslot"] <= (6 if p["loader"] else 2)
    # a context: pixel image, header words, packet words, destagger offsets, per-beam rows, in that order, inside ctx_bytes
    ends = [p["npix_instr"] * 1024, p["hdr_off"] + p["n_hdr"] * tw * 4, p["pkt_off"] + 6 * 256, p["off_off"] + -(-p["tr"] // 64) * 256,
            p["beam_off"] + -(-p["tr"] * 18 // 64) * 256]
    starts = [0, p["hdr_off"], p["pkt_off"], p["off_off"], p["beam_off"]]
    assert all(e <= s for e, s in zip(ends[:-1], starts[1:])) and ends[-1] <= p["ctx_bytes"] and p["ctx_bytes"] % 1024 == 0
    # slot i = [i * ctx_bytes, (i + 1) * ctx_bytes): disjoint by construction when the fixed area starts behind the last one
    assert p["fixed_off"] == p["nslot"] * p["ctx_bytes"]
    assert p["fixed_off"] + 3 * tw * 4 + 32 <= p["lds_bytes"]


def test_ring_layout_fits_for_every_static_profile(table):
    cases = [(s, W, H, tw, hts) for (s, W, H, tw) in _grid() for hts in (0, 1)]
    for knobs in ((), (("stream_slots", 2),), (("stream_slots", 3),), (("stream_slots", 6),)):
        plans = _plans([_line(table, s, W, H, tw, knobs=knobs, host_ts=hts) for s, W, H, tw, hts in cases])
        n_ok = 0
        for (s, W, H, tw, hts), p in zip(cases, plans):
            if not p["ok"]:
                continue
            n_ok += 1
            _check_layout(p, tw)
            if knobs:
                assert p["nslot"] == knobs[0][1]
            if p["loader"]:
                per = _dma_per_wave(p, tw, hts, True, 1)
                assert p["dma_per_tile"] == per, (s, W, H, tw, p)
                assert (p["nslot"] - 2) * max(per) <= 63, (s, W, H, tw, p)
            else:
                assert p["nslot"] == 2   # k_decode_stream, where every wave fetches, keeps its two contexts
        assert n_ok >= (10 if knobs != (("stream_slots", 6),) else 1), knobs


def test_plan_choice(table):
    """8 and 16 B/px keep two slots and the tallest tile; 12 B/px never goes below two passes of the workgroup, and a deeper ring
    is taken only where it keeps more packet bytes in flight than the tallest tile's two slots."""
    cases = _grid()
    own = _plans([_line(table, *c) for c in cases])
    two = _plans([_line(table, *c, knobs=(("stream_slots", 2),)) for c in cases])
    for (s, W, H, tw), p, q in zip(cases, own, two):
        assert p["ok"] == q["ok"], (s, W, H, tw)
        if not p["ok"]:
            continue
        rpp = 2048 // tw
        if s not in TWELVE:
            assert p == q, (s, W, H, tw)
        elif p["nslot"] > 2:
            assert p["tr"] >= 2 * rpp and p["tr"] <= q["tr"]
            assert (p["nslot"] - 1) * p["ctx_bytes"] > q["ctx_bytes"]
            assert p["key"] != q["key"]   # a verdict timed on the two-slot kernel is not applied to the ring
        else:
            assert p == q, (s, W, H, tw)


def test_two_slots_reproduce_the_recorded_stream_args(table):
    """nslot = 2 is the plan as it was recorded on an MI355X before the ring existed: SpecDualLB, SpecLB, SpecDual, field for field."""
    cols = table["columns"]
    lines, want = [], []
    for r in table["rows"]:
        c = dict(zip(cols, r))
        if c["stream"] < 0 or c["spec"] not in (1, 2, 4):
            continue
        i = {k: c[k] for k in cols[2:cols.index("sel")]}
        g = table["geometries"][c["geometry"]]
        kn = dict(table["knob_base"], **table["knobs"][c["knobs"]])
        tok = [f"g.{k}={v if not isinstance(v, list) else ','.join(map(str, v))}" for k, v in g.items()]
        tok += [f"k.{k}={v}" for k, v in kn.items()] + [f"{k}={v}" for k, v in i.items()]
        tok += [f"cus={table['device']['cus']}", f"resident_wgs={table['device']['resident_wgs']}", f"tw={c['cols']}"]
        for extra in ("", " k.stream_slots=2"):
            lines.append(" ".join(tok) + extra)
            want.append(table["streams"][c["stream"]])
    assert len(lines) >= 20
    for w, p in zip(want, _plans(lines)):
        assert p["ok"] and p["nslot"] == 2
        assert {k: p[k] for k in w} == w


def test_forced_depth_is_refused_not_clamped(table):
    # 128 x 2048 single return: two 128 x 32 contexts fill LDS; 128 x 16 fits five times, 256 x 8 four times, nothing six times
    lines = [_line(table, 3, 2048, 128, 128, knobs=(("stream_rows", 32), ("stream_slots", 3))),
             _line(table, 3, 2048, 128, 128, knobs=(("stream_slots", 6),)),
             _line(table, 3, 2048, 128, 256, knobs=(("stream_slots", 5),)),
             _line(table, 3, 2048, 128, 128, knobs=(("stream_slots", 7),)),
             _line(table, 3, 2048, 128, 128, knobs=(("stream_slots", 5),)),
             _line(table, 3, 2048, 128, 256, knobs=(("stream_slots", 4),)),
             _line(table, 3, 2048, 128, 128, knobs=(("stream_slots", 3), ("stream_loader", 0))),   # every wave fetches: two contexts only
             _line(table, 3, 2048, 128, 128, knobs=(("stream_slots", 3),), gate=1)]
    p = _plans(lines)
    assert [x["ok"] for x in p] == [0, 0, 0, 0, 1, 1, 0, 0]
    assert (p[4]["tr"], p[4]["nslot"]) == (16, 5) and (p[5]["tr"], p[5]["nslot"]) == (8, 4)


def test_gate_counts_keep_the_tall_tile(table):
    """Gate counts have one slot per row chunk (OUSTER_HIP_GATE_CHUNKS): the plan must not trade the tall tile for a ring there."""
    cases = [(s, W, H, tw) for (s, W, H, tw) in _grid() if s in TWELVE]
    plain = _plans([_line(table, *c, knobs=(("stream_slots", 2),)) for c in cases])
    gated = _plans([_line(table, *c, gate=1) for c in cases])
    for c, p, g in zip(cases, plain, gated):
        if g["ok"]:
            assert p["ok"] and g["tr"] == p["tr"] and g["nslot"] == 2 and g["loader"] == 0, c


# ---- the loader schedule, replayed ------------------------------------------------------------------------------------------
def _replay(nslot, n_mine, per_tile):
    """One loader wave and the decoders, in lock step at the per-tile barrier.  Returns the vmcnt operands of the waits.
    The wave's queue holds its DMA instructions in issue order; waiting for vmcnt <= k retires all but the youngest k."""
    queue = []            # tile index of every outstanding instruction, oldest first
    landed = set()        # tiles whose every instruction has retired
    last_read_done = {}   # slot -> tile whose reads of it are over (the decoders passed the next barrier)
    in_slot = {}
    waits = []

    def request(t):
        slot = t % nslot
        if slot in in_slot:   # refill: the tile that lived there must have been read to the end
            assert last_read_done.get(slot) == in_slot[slot], f"slot {slot} refilled before tile {in_slot[slot]} was read"
        in_slot[slot] = t
        queue.extend([t] * per_tile)

    def wait(k):
        waits.append(k)
        while len(queue) > k:
            t = queue.pop(0)
            if t not in queue:
                landed.add(t)

    issued = 0
    while issued < n_mine and issued + 1 < nslot:
        request(issued)
        issued += 1
    for it in range(n_mine):
        wait((issued - 1 - it) * per_tile)
        # barrier `it`: the decoders arrive having finished tile it - 1 and go on to read tile it
        if it:
            last_read_done[(it - 1) % nslot] = it - 1
        assert it in landed, f"tile {it} read before it landed"
        assert in_slot[it % nslot] == it
        if issued < n_mine:
            assert issued == it + nslot - 1   # the loader runs nslot - 1 tiles ahead
            request(issued)
            issued += 1
    assert issued == n_mine and all(t < n_mine for t in in_slot.values())   # nothing requested for tiles that do not exist
    return waits


@pytest.mark.parametrize("nslot", [2, 3, 4, 5, 6])
def test_loader_schedule(nslot):
    for per_tile in (1, 7, 63 // max(nslot - 2, 1)):
        for n_mine in range(0, 2 * nslot + 2):
            waits = _replay(nslot, n_mine, per_tile)
            assert len(waits) == n_mine and all(0 <= k <= 63 for k in waits)
            # constant in steady state, shorter counts only where the list runs out: never growing with the tile index
            assert all(a >= b for a, b in zip(waits, waits[1:])), waits
            if n_mine:
                assert waits[0] == (min(nslot - 1, n_mine) - 1) * per_tile and waits[-1] == 0
