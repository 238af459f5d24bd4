"""CPU-only: the decode launch plan (ouster_sdk_amd/csrc/decode_plan.cpp) against tests/golden/decode_plans.json.

Every row of the table is what ouster_hip_decode was about to launch for one set of inputs (geometry, knobs, counts,
alignments, CU count, the variant the tuner selected), recorded on an MI355X before the planner became a unit of its
own.  tests/cpp/plan_tool.cpp -- g++ only, no HIP library -- runs plan_candidates / tuner_key / plan_decode over the same
inputs; every recorded field must come out equal."""
import json
import os
import subprocess

import pytest

import cpp_tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "decode_plans.json")


def _line(row):
    i = row["in"]
    tok = [f"g.{k}={v if not isinstance(v, list) else ','.join(map(str, v))}" for k, v in i["g"].items()]
    tok += [f"k.{k}={v}" for k, v in i["knobs"].items()]
    tok += [f"{k}={v}" for k, v in i.items() if k not in ("g", "knobs")]
    tok.append(f"sel={row['sel']}")
    return " ".join(tok)


@pytest.fixture(scope="module")
def rows():
    with open(TABLE) as f:
        t = json.load(f)
    # rows are positional (t["columns"]); geometries, knob sets (as differences from knob_base), kernel names and StreamArgs are stored
    # once and referred to by index; the device values are the same for every row
    out = []
    for r in t["rows"]:
        c = dict(zip(t["columns"], r))
        i = {k: c[k] for k in t["columns"][2:t["columns"].index("sel")]}
        i.update(t["device"], g=t["geometries"][c["geometry"]], knobs=dict(t["knob_base"], **t["knobs"][c["knobs"]]))
        o = {k: c[k] for k in t["columns"][t["columns"].index("sel") + 1:-1]}
        o.update(kernel=t["kernels"][c["kernel"]], key=c["key"].rjust(16, "0"))
        if c["stream"] >= 0:
            o["stream"] = t["streams"][c["stream"]]
        out.append({"in": i, "sel": c["sel"], "out": o})
    return out


def _tool():
    """tests/cpp/_build/plan_tool, by the rule of tests/cpp/Makefile (g++ only): build() makes it, and this brings it up to date"""
    return cpp_tools.build("plan_tool")[0]


@pytest.fixture(scope="module")
def plans(rows):
    r = subprocess.run([_tool()], input="\n".join(_line(r) for r in rows) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


def test_plan_tool_links_no_hip_library():
    out = subprocess.run(["ldd", _tool()], capture_output=True, text=True).stdout.lower()
    assert "libc" in out and "hip" not in out and "hsa" not in out, out


def test_every_recorded_plan_is_reproduced(rows, plans):
    bad = []
    for n, (row, got) in enumerate(zip(rows, plans)):
        want = row["out"]
        for key, w in want.items():
            if key == "stream":
                for k2, w2 in w.items():
                    if got.get("stream", {}).get(k2) != w2:
                        bad.append((n, "stream." + k2, w2, got.get("stream", {}).get(k2)))
            elif got.get(key) != w:
                bad.append((n, key, w, got.get(key)))
        if "stream" not in want and "stream" in got:
            bad.append((n, "stream", None, got["stream"]))
    assert not bad, f"{len(bad)} fields differ, first: row {bad[0][0]} {bad[0][1]}: recorded {bad[0][2]!r}, planned {bad[0][3]!r}\n" + \
        _line(rows[bad[0][0]])


def test_narrow_fixup_launch_shape(rows, plans):
    """A fix-up pass on k_decode's tiles is a persistent grid: row_chunks = resident workgroups, tiles of the narrow width."""
    for row, got in zip(rows, plans):
        if row["out"]["fixup"] and not row["out"]["fix_wide"]:
            w, t = row["in"]["g"]["columns_per_frame"], row["out"]["narrow_tile"]
            assert got["fix_launch_shape"] == [0, row["in"]["resident_wgs"], 0, (w + t - 1) // t, 0]
        elif row["out"]["fix_wide"]:
            assert got["fix_launch_shape"] == row["out"]["fix_shape"]


def test_table_covers_what_it_must(rows):
    ins = [r["in"] for r in rows]
    outs = [r["out"] for r in rows]
    assert {i["spec"] for i in ins} >= {0, 1, 2, 3, 4, 5}                      # five static profiles + run-time descriptors
    assert {i["n_frames"] for i in ins} >= {1, 4, 16, 256, 512}
    home = [i["slots_per_frame"] * i["g"]["columns_per_packet"] == i["g"]["columns_per_frame"] for i in ins]
    assert any(home) and not all(home)                                          # one slot per column / compacted buffers
    assert {i["gate"] for i in ins} == {0, 1}
    assert {bool(i["poses"]) for i in ins} == {False, True}
    assert {i["xyzm"] for i in ins} >= {0, 1, 3}                                # no xyz, separable tables, full LUT
    assert {o["kernel"] for o in outs} >= {"k_decode", "k_decode_wide", "k_decode_stream", "k_decode_stream2", "k_decode_wide_resolved"}
    assert all(i["may_resolve"] for i, o in zip(ins, outs) if o["kernel"] == "k_decode_wide_resolved")   # recorded from an EXPERIMENTS=1 build
    knobs = {k: {i["knobs"][k] for i in ins} for k in ins[0]["knobs"]}
    assert knobs["wide"] >= {-1, 0, 128, 256} and knobs["stream"] >= {-1, 0, 128, 256}
    assert knobs["fixup_wide"] >= {0, 1} and knobs["slotmap"] >= {0, 1} and knobs["fixup"] >= {0, 1}
    assert {o["fixup"] for o in outs} == {0, 1} and {bool(o["fix_wide"]) for o in outs} == {False, True}
    assert {o["slotmap"] for o in outs} == {0, 1}
    assert any(len(o["candidates"]) == 5 for o in outs) and any(len(o["candidates"]) == 3 for o in outs)
    assert {r["sel"] for r in rows} >= {-1, 0, 128, 256, 1128, 1256}
