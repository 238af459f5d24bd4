"""GPU: the launch routes of the standalone kernels (k_destagger*, k_cartesian*, k_dewarp* of k_destagger / k_cartesian / k_dewarp.hip) that small,
aligned, power-of-two inputs never take, each against the CPU oracle.

Every test first asks the launch plan (ouster_sdk_amd/csrc/standalone_plan.cpp through tools/standalone_plan_tool) which route its
own inputs take and asserts that it is the intended one: a later change of a threshold fails the test instead of quietly
moving it onto a route that is tested elsewhere.

Bars are the project's own (tests/test_gpu_parity.py): destaggered planes bit-exact; separable tables < 1e-9 (f64) and
<= 4e-5 m (f32) against the double oracle; a full LUT bit-exact against O.cartesian with the LUT cast to the same type;
dewarp 1e-12 (f64) / 2e-5 (f32)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import standalone_plan_query as Q
from conftest import ROOT, has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch
    from ouster_sdk_amd import _capi as capi
    from ouster_sdk_amd.device import HotPath


def _np(t):
    return t.cpu().numpy()


def _misaligned(a, off):
    """A contiguous CUDA tensor with the content of `a` that starts `off` bytes into its allocation."""
    raw = np.zeros(off + a.nbytes, dtype=np.uint8)
    raw[off:] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.uint32, np.dtype(np.float32): torch.float32,
           np.dtype(np.float64): torch.float64}[a.dtype]
    t = torch.from_numpy(raw).cuda()[off:].view(tdt).reshape(a.shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == off
    return t


def _cartesian_into_nan(hp, lut, rng_ptr, n, tdt, out=None, first=0):
    """ouster_hip_cartesian on n images from rng_ptr; the output starts as NaN, so a pixel nobody wrote shows."""
    npix = hp.h * hp.w
    if out is None:
        out = torch.full((n, npix, 3), float("nan"), dtype=tdt, device="cuda")
        first = 0
    capi.check(hp.ctx.L.ouster_hip_cartesian(hp.ctx.h, lut.h, rng_ptr, out.data_ptr() + first * npix * 3 * out.element_size(),
                                             capi.F32 if tdt == torch.float32 else capi.F64, n))
    return out


def _ranges(rng, n, h, w):
    r = rng.integers(0, 2 ** 19, size=(n, h, w)).astype(np.uint32)
    r[rng.random(r.shape) < 0.3] = 0
    return r


def _calib(O, h, w):
    cal = O.synthetic_calib(h=h, w=w, b2l_x=15.806)
    ext = np.eye(4)
    ext[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    ext[:3, 3] = [1.5, -2.0, 0.25]
    cal.extrinsic = ext
    return cal


class _Cart:
    """One geometry: the separable LUT and both full LUTs on the device, and the oracle's answer per mode."""
    MODES = {"sep32": ("sep", np.float64, "f32"), "sep64": ("sep", np.float64, "f64"),
             "full32": ("full32", np.float32, "f32"), "full64": ("full64", np.float64, "f64")}

    def __init__(self, O, h, w, cpp):
        self.O, self.h, self.w = O, h, w
        cal = _calib(O, h, w)
        self.ldir, self.lofs = cal.xyz_lut(True)
        self.hp = HotPath("RNG15_RFL8_NIR8", h, w, cpp)
        self.luts = {"sep": self.hp.add_lut(cal.beam_to_lidar, cal.lut_transform(True), cal.beam_azimuth_angles,
                                            cal.beam_altitude_angles),
                     "full32": self.hp.add_lut_arrays(self.ldir.astype(np.float32), self.lofs.astype(np.float32)),
                     "full64": self.hp.add_lut_arrays(self.ldir, self.lofs)}

    def want(self, r, mode):
        """[n, h*w, 3]: the double oracle for the separable modes, O.cartesian with the LUT cast to its type for the full ones."""
        ldt = self.MODES[mode][1]
        return np.stack([self.O.cartesian(x, self.ldir.astype(ldt), self.lofs.astype(ldt)) for x in r])

    def lut(self, mode):
        return self.luts[self.MODES[mode][0]]

    def tdt(self, mode):
        return torch.float32 if self.MODES[mode][2] == "f32" else torch.float64

    def check(self, got, want_d, mode, what):
        """got against the expectation, both on the device, by the bar of the mode."""
        assert not torch.isnan(got).any(), (what, mode, "pixels nobody wrote")
        if mode.startswith("full"):
            assert want_d.dtype == got.dtype
            assert torch.equal(got, want_d), (what, mode)
        else:
            err = float((got.double() - want_d).abs().max())
            print(f"{what} {mode}: max |dxyz| = {err:.3e}")
            assert (err < 1e-9) if mode == "sep64" else (err <= 4e-5), (what, mode, err)


# ------------------------------------------------------------------------------------------------------------------
# k_cartesian_tiled with 2 / 4 / 8 / 16 images per workgroup
# ------------------------------------------------------------------------------------------------------------------
GH, GW, NBASE = 20, 68, 37   # one full 64-column tile + a ragged one whose only live lane is q = 0; rows_per_block 32 > h
EXTRA = {2: 1, 4: 3, 8: 5, 16: 7}   # images of the last, partial group: never a multiple of 4


@pytest.fixture(scope="module")
def grouped(oracle):
    """37 distinct base images (coprime with 4 and 16: neighbours within a group always differ) and the oracle's answer
    for them per mode, resident on the device; image i of a batch is base[i % 37]."""
    c = _Cart(oracle, GH, GW, 4)
    rng = np.random.default_rng(68020)
    base = _ranges(rng, NBASE, GH, GW)
    base[0, 0, :8] = 2 ** 19 - 8      # max range
    base[1, GH - 1, GW - 4:] = 1      # the ragged tile's quad, last row
    base[2, 0, 60:] = [1, 2 ** 19 - 8, 0, 1, 2 ** 19 - 8, 1, 0, 2 ** 19 - 8]   # across the tile boundary
    assert (base == 0).mean() > 0.25 and (base == 1).any() and (base == 2 ** 19 - 8).any()
    c.base_d = torch.from_numpy(base.view(np.int32)).cuda()
    c.want_d = {m: torch.from_numpy(c.want(base, m)).cuda() for m in ("sep64", "full32")}
    c.want_d["sep32"] = c.want_d["sep64"]
    c.want_d["full64"] = c.want_d["sep64"]   # O.cartesian with the double LUT is both the oracle and cartesianT<double>
    return c


@pytest.mark.parametrize("mode,group", [("full32", 2), ("full32", 4), ("full32", 8), ("full32", 16),   # the benchmark's row: the whole ladder
                                        ("sep32", 4), ("sep32", 16), ("sep64", 2), ("sep64", 16),
                                        ("full64", 8), ("full64", 16)])
def test_cartesian_grouped_images(grouped, mode, group):
    """k_cartesian_tiled's project_group: `group` images per workgroup, walked four at a time with a four-deep prefetch;
    the last group is partial and not a multiple of 4 (16: one full pass of four, then three).
    Wall time of the largest case (16 images per workgroup, 16391 images, 22.3 M pixels) on an MI355X: see the print."""
    c = grouped
    t0 = time.perf_counter()
    n_min = Q.smallest_n_for_group(GW, GH, group)
    assert Q.cartesian(GW, GH, n_min - 1)["images_per_block"] == group // 2
    n = (n_min + group - 1) // group * group + EXTRA[group]
    plan = Q.cartesian(GW, GH, n)
    assert plan["route"] == "TILED" and plan["images_per_block"] == group and plan["rows_per_block"] == 32 > GH, plan
    assert n % group == EXTRA[group] and EXTRA[group] % 4 != 0 and plan["grid"] == [2, n // group + 1]
    eight = [Q.cartesian(GW, GH, k) for k in (8, n % 8)]
    assert all(p["route"] == "TILED" and p["images_per_block"] == 1 for p in eight), eight

    npix = GH * GW
    idx = torch.arange(n, device="cuda") % NBASE
    r = c.base_d[idx].contiguous()                       # int32 view of the uint32 ranges
    assert r.data_ptr() % 16 == 0 and r.shape == (n, GH, GW)
    tdt = c.tdt(mode)
    got = _cartesian_into_nan(c.hp, c.lut(mode), r.data_ptr(), n, tdt)
    c.check(got, c.want_d[mode][idx], mode, f"{group} images per workgroup, n={n}")
    # not the reference, a second witness: the same images eight at a time (one image per workgroup) give the same bytes
    by8 = torch.full_like(got, float("nan"))
    for i in range(0, n, 8):
        _cartesian_into_nan(c.hp, c.lut(mode), r.data_ptr() + i * npix * 4, min(8, n - i), tdt, out=by8, first=i)
    ity = torch.int32 if tdt == torch.float32 else torch.int64
    assert torch.equal(got.view(ity), by8.view(ity)), (mode, group)
    torch.cuda.synchronize()
    print(f"cartesian {mode}, {group} images per workgroup, {n} images: {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------------------------
# the generic k_cartesian
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,off", [(4, 33, 0),    # aligned, h*w % 4 == 0, w % 4 != 0: a 16 B quad straddles a row boundary
                                     (7, 36, 4)])   # w % 4 == 0, range 4 bytes off alignment: vec false, every quad full
def test_cartesian_generic_kernel(oracle, h, w, off):
    n = 3
    c = _Cart(oracle, h, w, 4 if w % 4 == 0 else 1)
    rng = np.random.default_rng(h * 10007 + w)
    r = _ranges(rng, n, h, w)
    r[0, 0, :4] = 2 ** 19 - 8
    r[1, h - 1, w - 3:] = [1, 2 ** 19 - 8, 1]
    dr = _misaligned(r, off)
    vec_ok = dr.data_ptr() % 16 == 0 and (h * w) % 4 == 0     # ouster_hip_cartesian's own rule (the output is aligned)
    assert vec_ok == (off == 0)
    plan = Q.cartesian(w, h, n, vec_ok)
    assert plan["route"] == "GENERIC", plan
    if off:                                                   # the misaligned pointer alone is what takes it off the tiled kernel
        assert Q.cartesian(w, h, n, True)["route"] == "TILED"
    else:
        assert w % 4 != 0 and (h * w) % 4 == 0 and (h * w * 4) % 16 == 0
    for mode in ("sep32", "sep64", "full32", "full64"):
        got = _cartesian_into_nan(c.hp, c.lut(mode), dr.data_ptr(), n, c.tdt(mode))
        assert got.data_ptr() % 16 == 0
        c.check(got, torch.from_numpy(c.want(r, mode)).cuda(), mode, f"generic {h}x{w} +{off} B")


# ------------------------------------------------------------------------------------------------------------------
# the generic k_dewarp<T>
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,off,tol", [(np.float32, 4, 2e-5), (np.float64, 8, 1e-12)])
def test_dewarp_generic_kernel_behind_a_misaligned_pointer(oracle, dt, off, tol):
    O = oracle
    h, w, n = 7, 36, 3
    rng = np.random.default_rng(736 + off)
    hp = HotPath("RNG15_RFL8_NIR8", h, w, 4)
    poses = np.tile(np.eye(4), (n, w, 1, 1))
    ang = rng.uniform(-0.3, 0.3, size=(n, w))
    poses[..., 0, 0] = np.cos(ang); poses[..., 0, 2] = np.sin(ang)
    poses[..., 2, 0] = -np.sin(ang); poses[..., 2, 2] = np.cos(ang)
    poses[..., :3, 3] = rng.uniform(-5, 5, size=(n, w, 3))
    pts = rng.uniform(-100, 100, size=(n, h * w, 3)).astype(dt)
    d_pts = _misaligned(pts, off)
    assert Q.dewarp(w, h, n, aligned=False)["route"] == "GENERIC" and Q.dewarp(w, h, n, aligned=True)["route"] == "TILED"
    got = hp.dewarp(d_pts, torch.from_numpy(poses).cuda())
    assert got.data_ptr() % 16 == 0                          # the points alone are off alignment
    want = np.stack([O.dewarp(pts[k], poses[k], h, w) for k in range(n)])
    err = np.abs(_np(got).astype(np.float64) - want.astype(np.float64)).max()
    print(f"generic dewarp {dt.__name__}: max err {err:.3e}")
    assert err <= tol


# ------------------------------------------------------------------------------------------------------------------
# destagger
# ------------------------------------------------------------------------------------------------------------------
def _shift_passes(w, h, seed):
    """Shift vectors of h rows that between them hold 0, +-1, +-(w-1), +-w, w+3, -(2w+5) -- the size_t arithmetic of
    dest_offsets for |s| >= w -- then +-2 (with +-1: all four byte phases of an 8-bit row) and random values."""
    s = [0, 1, -1, w - 1, -(w - 1), w, -w, w + 3, -(2 * w + 5), 2, -2]
    rng = np.random.default_rng(seed)
    s += list(rng.integers(-w + 1, w, (-len(s)) % h))
    a = np.array(s, dtype=np.int32).reshape(-1, h)
    assert {0, 1, -1, w - 1, 1 - w, w, -w, w + 3, -2 * w - 5} <= set(a.reshape(-1).tolist())
    return a


def _rows_env():
    e = os.environ.get("OUSTER_HIP_DESTAGGER_ROWS")
    try:
        return int(e) if e else -1
    except ValueError:
        return 0


def _check_destagger(O, img, got_by_pass, passes, w):
    """img [n, h, w, elem] bytes; got_by_pass[p][inverse] the device's answer for shift vector p."""
    for p, shifts in enumerate(passes):
        for inverse in (False, True):
            got = got_by_pass[p][int(inverse)]
            for k in range(img.shape[0]):
                assert np.array_equal(got[k], O.destagger(img[k], shifts, inverse)), (p, inverse, k, shifts)
                if (w & (w - 1)) == 0:   # power-of-two widths: equals np.roll (reference.py:131-158)
                    roll = np.stack([np.roll(img[k][u], (-1 if inverse else 1) * int(shifts[u]), axis=0)
                                     for u in range(img.shape[1])])
                    assert np.array_equal(got[k], roll), (p, inverse, k)


# elem bytes, w, h, bytes off alignment, the route the launch takes
DESTAGGER_CASES = [
    pytest.param(2, 4096, 5, 0, "LDS", id="uint16-w4096-8KB-lds-funnel-shift"),
    pytest.param(1, 8192, 5, 0, "LDS", id="uint8-w8192-8KB-lds-four-byte-phases"),
    pytest.param(6, 2048, 3, 0, "LDS", id="uint16x3-w2048-12KB-lds"),
    pytest.param(6, 16384, 3, 0, "DIRECT", id="uint16x3-w16384-96KB-direct-funnel-shift"),
    pytest.param(24, 4096, 3, 0, "DIRECT", id="float64x3-w4096-96KB-direct-straddle"),
    pytest.param(1, 1024, 5, 0, "ROWS1", id="uint8-w1024-two-rows-odd-h"),
    pytest.param(2, 2048, 7, 0, "ROWS1", id="uint16-w2048-two-rows-odd-h"),
    pytest.param(4, 1024, 5, 4, "BYTES", id="uint32-w1024-source-4B-off-bytes"),
    pytest.param(4, 1000, 5, 0, "ROWS1", id="uint32-w1000"),
    pytest.param(1, 999, 5, 0, "BYTES", id="uint8-w999"),
]


@pytest.mark.parametrize("elem,w,h,off,route", DESTAGGER_CASES)
def test_destagger_routes(oracle, elem, w, h, off, route):
    O = oracle
    n = 3
    plan = Q.destagger(w * elem, aligned=off == 0, rows_env=_rows_env(), h=h, n=n)
    assert plan["route"] == route, plan
    if route.startswith("ROWS"):      # an odd h: the last workgroup holds one row
        assert plan["rows_per_wg"] == 2 and h % 2 == 1 and plan["grid"] == [(h + 1) // 2, n]
    if off:                           # the 16 B granular row alone would have taken a vector route
        assert (w * elem) % 16 == 0 and Q.destagger(w * elem, True, _rows_env(), h, n)["route"] != "BYTES"
    passes = _shift_passes(w, h, seed=w * 31 + elem)
    if elem == 1 and route == "LDS":
        assert {int(s) % 4 for s in passes.reshape(-1)} == {0, 1, 2, 3}
    img = np.random.default_rng(elem * 1000003 + w).integers(0, 256, size=(n, h, w, elem), dtype=np.uint8)
    d_img = _misaligned(img, off)
    hp = HotPath("RNG15_RFL8_NIR8", 128, 1024, 16)
    got = []
    for shifts in passes:
        fwd = hp.destagger(d_img, shifts)
        assert fwd.data_ptr() % 16 == 0
        got.append((_np(fwd), _np(hp.destagger(d_img, shifts, inverse=True))))
        if (w & (w - 1)) == 0:   # round trip: stagger(destagger(x)) == x
            assert torch.equal(hp.destagger(fwd, shifts, inverse=True), d_img), shifts
    _check_destagger(O, img, got, passes, w)


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from ouster_sdk_amd.device import HotPath
z = np.load(sys.argv[2])
hp = HotPath("RNG15_RFL8_NIR8", 128, 1024, 16)
out = {}
for key in ("a", "b"):
    d = torch.from_numpy(z["img_" + key]).cuda()
    assert d.data_ptr() % 16 == 0
    for p, shifts in enumerate(z["passes_" + key]):
        for inverse in (0, 1):
            out[f"{key}_{p}_{inverse}"] = hp.destagger(d, shifts, inverse=bool(inverse)).cpu().numpy()
hp.sync()
np.savez(sys.argv[3], **out)
"""


def test_destagger_rows_2_and_4_in_a_child_process(oracle, tmp_path):
    """k_destagger_rows<2> and <4> are reachable only through OUSTER_HIP_DESTAGGER_ROWS, which a process reads once: one fresh
    child with the variable set to 3 destaggers 8 KB rows (<2>) and 16 KB rows (<4>) of 7 rows (3 + 3 + 1 per workgroup)."""
    O = oracle
    n, h = 3, 7
    cases = {"a": (2048, "ROWS2"), "b": (4096, "ROWS4")}      # uint32
    data = {}
    for key, (w, route) in cases.items():
        plan = Q.destagger(w * 4, True, 3, h, n)
        assert plan["route"] == route and plan["rows_per_wg"] == 3 and plan["grid"] == [3, n] and plan["lds_bytes"] == 2 * w * 4, plan
        data["img_" + key] = np.random.default_rng(w).integers(0, 256, size=(n, h, w, 4), dtype=np.uint8)
        data["passes_" + key] = _shift_passes(w, h, seed=w + 7)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **data)
    env = dict(os.environ, OUSTER_HIP_DESTAGGER_ROWS="3")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, src, dst], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(dst)
    for key, (w, _) in cases.items():
        passes = data["passes_" + key]
        got = [(out[f"{key}_{p}_0"], out[f"{key}_{p}_1"]) for p in range(len(passes))]
        _check_destagger(O, data["img_" + key], got, passes, w)
