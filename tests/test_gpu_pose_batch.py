"""interp_poses on a resident hip::DeviceFrameBatch, through tests/cpp/pose_batch_tool.cpp: 5 frames of the two small sensors of
the frame_ops batch test, one packet of one frame left out, column timestamps near 1.7e9 s, a trajectory of 9 known poses
spanning the 5 frames.  Valid columns must carry the pose of tests/pose_model.py at timestamp * 1e-9 s within the bound of
tests/golden/make_pose_golden.py (computed here for this very case: long-double truth, the float64 model's own error as the
unit); the missing packet's columns keep their bits -- identity on a fresh batch, the uploaded poses on the second one;
dewarp() after interp_poses equals dewarp() of a batch that got the same poses through download_poses -> upload_poses, for a
float batch (which reads the float rows written by the same launch) and for an xyz_f64 batch.  The C ABI's column form is
checked on its own for the float rows and the untouched bytes."""
import numpy as np
import pytest

import cpp_tools
import pose_model as M
from batch_cases import COL_NS, FRAME_NS, H, K, N, SKIP_FRAME, SKIP_PACKET, T0_NS, W, write_known, write_packets
from conftest import has_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run(oracle, tmp_path_factory):
    assert has_gpu()
    tmp = tmp_path_factory.mktemp("pose_batch")
    write_packets(oracle, tmp)
    xk, poses = write_known(tmp)
    res = cpp_tools.run("pose_batch_tool", [tmp / "packets.bin", H, W, N, SKIP_FRAME, SKIP_PACKET, tmp / "known.bin", K, tmp / "o", "1.0", "200.0"])
    out = {"stdout": res.stdout, "xk": xk, "poses": poses}
    for tag in ("f32", "f64"):
        raw = np.fromfile(tmp / ("o.%s.hdr" % tag), np.uint8)
        ts = raw[:N * W * 8].view(np.uint64).reshape(N, W)
        st = raw[N * W * 8:].view(np.uint32).reshape(N, W)
        out[tag] = dict(ts=ts, status=st, **{p: np.fromfile(tmp / ("o.%s.%s" % (tag, p)), np.float64).reshape(N, W, 16) for p in ("p0", "p1", "p2")})
    # the yardstick, once for both batches: the valid columns' times, the truth and the unit of the bound
    ts, st = out["f64"]["ts"], out["f64"]["status"]
    valid = (st & 1) != 0
    x = ts[valid].astype(np.float64) * 1e-9
    order = np.argsort(x, kind="stable")
    inv = np.argsort(order)
    xs = x[order]
    for name, compute in (("general", lambda dt: M.interp_pose(xs, xk, poses, dt)),
                          ("pair", lambda dt: M.interp_pose_two(xs, xk[0], poses[0], xk[-1], poses[-1], dt))):
        truth = compute(np.longdouble).astype(np.float64).reshape(-1, 16)[inv]
        model = compute(np.float64).reshape(-1, 16)[inv]
        scale = max(1.0, float(np.abs(poses).max()), float(np.abs(truth).max()))
        model_err = float(np.abs(model - truth).max() / (M.EPS * scale))
        out[name] = dict(truth=truth, lim=M.bound(None, model_err, scale), model_err=model_err, unit=M.EPS * scale)
    out["valid"], out["x"] = valid, x
    out["rows2"] = np.fromfile(tmp / "o.f32.rows2", np.float32).reshape(N, W, 12)
    # what the tool put into the invalid columns of the second batch before upload_poses
    marker = np.tile(poses[-1], (N, W, 1))
    marker[:, :, 3] += 0.5 * (np.arange(W)[None, :] + 1)
    marker[:, :, 7] -= np.arange(N)[:, None]
    out["marker"] = marker
    return out


def test_headers_are_what_the_test_encoded(run):
    for tag in ("f32", "f64"):
        ts, st = run[tag]["ts"], run[tag]["status"]
        missing = np.zeros((N, W), bool)
        missing[SKIP_FRAME, SKIP_PACKET * 16:(SKIP_PACKET + 1) * 16] = True
        assert np.array_equal((st & 1) == 0, missing)
        want = T0_NS + np.arange(N)[:, None] * FRAME_NS + np.arange(W)[None, :] * COL_NS
        assert np.array_equal(ts[~missing], want.astype(np.uint64)[~missing])
    segs = {M.segment_index(run["xk"], x) for x in run["x"]}
    assert len(segs) >= 5   # the frames fall into different segments
    assert run["general"]["model_err"] <= 64.0 and run["pair"]["model_err"] <= 64.0   # the case is inside the maker's condition


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_fresh_batch_has_identity_poses(run, tag):
    assert np.array_equal(run[tag]["p0"], np.tile(np.eye(4).reshape(16), (N, W, 1)))


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_valid_columns_get_the_model_pose_and_the_others_keep_theirs(run, tag):
    valid, y = run["valid"], run["general"]
    got = run[tag]["p1"]
    err = float(np.abs(got[valid] - y["truth"]).max())
    print("%s: max |pose - truth| = %.3g = %.2f eps x scale (allowed %.3g, model_err %.2f)" % (tag, err, err / y["unit"], y["lim"], y["model_err"]))
    assert err <= y["lim"]
    assert (~valid).sum() == 16
    assert got[~valid].tobytes() == np.tile(np.eye(4).reshape(16), (16, 1)).tobytes()      # identity, bit for bit
    # frames in different segments get different poses; columns of one frame differ too
    assert not np.array_equal(got[0, 0], got[4, 0]) and not np.array_equal(got[0, 0], got[0, 1])


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_two_pose_overload_over_uploaded_poses(run, tag):
    """The second batch got its poses through upload_poses, a marker pose in the invalid columns: the two-pose interp_poses must
    leave exactly those 128 B (and, in a float batch, the 48 B of float rows dewarp() reads) as upload_poses wrote them."""
    valid, y = run["valid"], run["pair"]
    got, before, marker = run[tag]["p2"], run[tag]["p1"], run["marker"]
    err = float(np.abs(got[valid] - y["truth"]).max())
    print("%s: pair form max |pose - truth| = %.3g = %.2f eps x scale (allowed %.3g)" % (tag, err, err / y["unit"], y["lim"]))
    assert err <= y["lim"]
    assert (~valid).sum() == 16
    assert got[~valid].tobytes() == marker[~valid].tobytes()                # the uploaded marker, bit for bit
    assert not np.array_equal(marker[~valid], before[~valid])               # ... which is not the identity the first batch kept
    assert len({r.tobytes() for r in marker[~valid]}) == 16                  # ... and differs from column to column
    assert not np.array_equal(got[valid], before[valid])
    if tag == "f32":
        rows = run["rows2"]
        assert rows[~valid].tobytes() == marker[~valid][:, :12].astype(np.float32).tobytes()
        assert rows[valid].tobytes() == got[valid][:, :12].astype(np.float32).tobytes()


def test_dewarp_after_interp_poses_equals_the_upload_route(run):
    for tag in ("f32", "f64"):
        assert "dewarp_equal %s 1" % tag in run["stdout"], run["stdout"]
        assert "poses_matter %s 1" % tag in run["stdout"], run["stdout"]
        points = [int(ln.split()[2]) for ln in run["stdout"].splitlines() if ln.startswith("points " + tag)]
        assert points and points[0] > N * W   # the gate keeps a real cloud


def test_column_form_of_the_c_abi_writes_float_rows_and_nothing_else(run):
    import torch
    from ouster_sdk_amd import _capi as capi
    ctx = capi.Context(0)
    try:
        ts, st = run["f64"]["ts"], run["f64"]["status"].copy()
        st[1, 5] = 0xFFFFFFFE   # bit 0 clear under other bits: skipped
        st[2, 7] = 3            # bit 0 set among others: computed
        xk, poses = run["xk"], run["poses"]
        d_ts, d_st = torch.from_numpy(ts.view(np.int64)).cuda(), torch.from_numpy(st.view(np.int32)).cuda()
        guard = 256
        d_p = torch.full((guard + N * W * 128 + guard,), 0xCD, dtype=torch.uint8, device="cuda")
        d_r = torch.full((guard + N * W * 48 + guard,), 0xCD, dtype=torch.uint8, device="cuda")
        capi.check(ctx.L.ouster_hip_interp_pose_columns(ctx.h, d_ts.data_ptr(), d_st.data_ptr(), N, W, xk.ctypes.data, poses.ctypes.data,
                                                        K, d_p.data_ptr() + guard, d_r.data_ptr() + guard))
        ctx.sync()
        p, r = d_p.cpu().numpy(), d_r.cpu().numpy()
        assert np.all(p[:guard] == 0xCD) and np.all(p[-guard:] == 0xCD) and np.all(r[:guard] == 0xCD) and np.all(r[-guard:] == 0xCD)
        p8, r8 = p[guard:-guard].reshape(N, W, 128), r[guard:-guard].reshape(N, W, 48)
        valid = (st & 1) != 0
        assert (~valid).sum() == 17
        assert np.all(p8[~valid] == 0xCD) and np.all(r8[~valid] == 0xCD)
        pd, rf = p8[valid].copy().view(np.float64).reshape(-1, 16), r8[valid].copy().view(np.float32).reshape(-1, 12)
        assert rf.tobytes() == pd[:, :12].astype(np.float32).tobytes()
        same = valid & ((run["f64"]["status"] & 1) != 0)
        assert p8[same].tobytes() == run["f64"]["p1"].view(np.uint8).reshape(N, W, 128)[same].tobytes()   # the batch ran the same launch
        # without rows: the poses alone, the same bits
        d_q = torch.full((N * W * 128,), 0xCD, dtype=torch.uint8, device="cuda")
        capi.check(ctx.L.ouster_hip_interp_pose_columns(ctx.h, d_ts.data_ptr(), d_st.data_ptr(), N, W, xk.ctypes.data, poses.ctypes.data,
                                                        K, d_q.data_ptr(), None))
        ctx.sync()
        assert d_q.cpu().numpy().tobytes() == p[guard:-guard].tobytes()
        # the direct-store form (knob "pose_direct"): the same bytes everywhere, skipped columns and guards included
        ctx.set_knob("pose_direct", 1)
        d_p2 = torch.full_like(d_p, 0xCD)
        d_r2 = torch.full_like(d_r, 0xCD)
        capi.check(ctx.L.ouster_hip_interp_pose_columns(ctx.h, d_ts.data_ptr(), d_st.data_ptr(), N, W, xk.ctypes.data, poses.ctypes.data,
                                                        K, d_p2.data_ptr() + guard, d_r2.data_ptr() + guard))
        ctx.sync()
        assert d_p2.cpu().numpy().tobytes() == p.tobytes() and d_r2.cpu().numpy().tobytes() == r.tobytes()
    finally:
        ctx.close()
