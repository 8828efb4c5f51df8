"""TSDF fusion, the host side (include/sage_ba.h "TSDF fusion"): sage_tsdf_frustum_bounds and sage_tsdf_plan against the numpy
expressions of the script's own arithmetic (generate_reconstruction_fly_through.py:376-387, :561-574, :138-143, restated), to
1e-12 relative, and every SAGE_E_INVALID of the planning, volume and integrate calls that can be answered with no device
present.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sage_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, STATE = -1, -2, -4
NEW = ["sage_tsdf_frustum_bounds", "sage_tsdf_plan", "sage_tsdf_create", "sage_tsdf_destroy", "sage_tsdf_reset", "sage_tsdf_get",
       "sage_tsdf_dev", "sage_tsdf_integrate", "sage_tsdf_integrate_batch", "sage_tsdf_integrate_batch_launches",
       "sage_tsdf_view_chunk", "sage_tsdf_last_stats", "sage_window_depth_range", "sage_window_fuse_tsdf"]


@pytest.fixture(scope="module")
def capi():
    from sage_slam_amd import capi as c
    c.lib()
    return c


def test_symbols_are_declared_exported_and_bound(capi):
    hdr = open(os.path.join(ROOT, "include", "sage_ba.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name), name


def script_frustum(cam, pose12, max_depth):
    """get_view_frustum: five points, camera to world"""
    w, h = float(cam.w), float(cam.h)
    fx, fy, cx, cy = (float(np.float32(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    d = np.array([0, max_depth, max_depth, max_depth, max_depth], np.float64)
    pts = np.array([(np.array([0, 0, 0, w, w]) - cx) * d / fx, (np.array([0, 0, h, 0, h]) - cy) * d / fy, d])
    P = np.asarray(pose12, np.float32).astype(np.float64)
    return P[:9].reshape(3, 3) @ pts + P[9:].reshape(3, 1)


def test_frustum_bounds_and_plan_follow_the_script(capi):
    rng = np.random.default_rng(3)
    scene = synth.make_tsdf_scene(5, n=6)
    cam = scene["cam"]
    bnds = np.zeros((3, 2))
    mine = np.zeros(6)
    for v in scene["views"]:
        md = float(v["depth"].max()) + float(rng.uniform(0, 1))
        pts = script_frustum(cam, v["pose12"], md)
        bnds[:, 0] = np.minimum(bnds[:, 0], np.amin(pts, axis=1))
        bnds[:, 1] = np.maximum(bnds[:, 1], np.amax(pts, axis=1))
        mine = capi.tsdf_frustum_bounds(cam, v["pose12"], md, mine)
        want = np.concatenate([bnds[:, 0], bnds[:, 1]])
        assert np.all(np.abs(mine - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    assert np.all(mine[:3] <= 0) and np.all(mine[3:] >= 0)                       # zeros at the start: the world origin is inside
    own = capi.tsdf_frustum_bounds(cam, scene["views"][0]["pose12"], 1.0, [np.inf] * 3 + [-np.inf] * 3)
    pts = script_frustum(cam, scene["views"][0]["pose12"], 1.0)
    assert np.allclose(own, np.concatenate([pts.min(1), pts.max(1)]), rtol=1e-12, atol=0)
    for max_voxels, mult in ((64.0e6, 10.0), (5.0e4, 3.0), (0.0, 2.0)):
        base = 0.1
        voxel = base
        if max_voxels > 0:
            vol_dim = (bnds[:, 1] - bnds[:, 0]) / base
            voxel = base * (vol_dim[0] * vol_dim[1] * vol_dim[2] / max_voxels) ** (1.0 / 3.0)
        dim = np.ceil((bnds[:, 1] - bnds[:, 0]) / voxel).astype(int)
        p = capi.tsdf_plan(mine, base, max_voxels, mult, with_color=True)
        assert abs(p.voxel_size - voxel) <= 1e-12 * voxel + np.spacing(np.float32(voxel))      # (an fp32 field)
        assert list(p.dim) == list(dim) and p.voxels == int(np.prod(dim))
        assert np.array_equal(np.array(p.origin[:], np.float32), bnds[:, 0].astype(np.float32))
        assert p.trunc_margin == np.float32(voxel * mult) or abs(p.trunc_margin - voxel * mult) <= np.spacing(np.float32(voxel * mult))
        assert p.with_color == 1 and p.device_bytes >= 12 * p.voxels
        if max_voxels > 0:
            assert p.voxels <= 1.2 * max_voxels + 3 * max(dim) ** 2                 # ceil adds at most a layer per axis


def test_plan_refusals(capi):
    out = capi.SageTsdfPlan()
    good = np.array([0, 0, 0, 1, 1, 1], np.float64)

    def plan(b, base=0.1, mv=1e6, mult=3.0, o=out):
        b = None if b is None else np.ascontiguousarray(b, np.float64)
        return capi.tsdf_plan_raw(None if b is None else b.ctypes.data, base, mv, mult, 0, None if o is None else C.addressof(o))

    assert plan(good) == 0
    assert plan(None) == INVALID and plan(good, o=None) == INVALID
    assert plan([0, 0, 0, 1, 0, 1]) == INVALID and plan([0, 0, 2, 1, 1, 1]) == INVALID      # empty along an axis
    assert plan([0, 0, 0, 1, np.nan, 1]) == INVALID and plan([-np.inf, 0, 0, 1, 1, 1]) == INVALID
    assert plan(good, base=0.0) == INVALID and plan(good, base=np.nan) == INVALID and plan(good, mult=0.0) == INVALID
    assert plan(good, mv=np.nan) == INVALID
    assert plan([0, 0, 0, 1300, 1300, 1300], base=1.0, mv=0.0) == INVALID                   # 2.197e9 voxels > 2^31 - 1
    assert plan([0, 0, 0, 1290, 1290, 1290], base=1.0, mv=0.0) == 0                         # 2.147e9 < 2^31 - 1
    assert plan([0, 0, 0, 1, 1, 1], base=1e-12, mv=0.0) == INVALID


def test_frustum_refusals(capi):
    cam = capi.SageCamera(30.0, 30.0, 15.5, 11.5, 32.0, 24.0)
    pose = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(np.float32)
    b = np.zeros(6)

    def call(c=cam, p=pose, md=1.0, bb=b):
        return capi.tsdf_frustum_bounds_raw(None if c is None else C.addressof(c), None if p is None else p.ctypes.data, md,
                                            None if bb is None else bb.ctypes.data)

    assert call() == 0
    assert call(c=None) == INVALID and call(p=None) == INVALID and call(bb=None) == INVALID
    assert call(md=np.nan) == INVALID and call(md=np.inf) == INVALID
    for field, bad in (("fx", 0.0), ("fy", -1.0), ("w", 0.0), ("h", 0.5), ("cx", np.nan)):
        c2 = capi.SageCamera(30.0, 30.0, 15.5, 11.5, 32.0, 24.0)
        setattr(c2, field, bad)
        assert call(c=c2) == INVALID, field
    p2 = pose.copy(); p2[4] = np.inf
    assert call(p=p2) == INVALID


class FakeTensor:
    """an address that is never read: the calls below refuse before they touch the device"""

    def __init__(self, n):
        self.n = n

    def data_ptr(self):
        return 4096

    def numel(self):
        return self.n


def test_volume_and_integrate_refusals_without_a_device(capi):
    L = capi.lib()
    plan = capi.tsdf_plan_exact((8, 8, 8), (0, 0, 0), 0.1, 0.3)
    h = C.c_void_p()
    assert capi.tsdf_create_raw(None, C.addressof(plan), C.addressof(h)) == INVALID
    fake = C.c_void_p(4096)                                                    # never dereferenced: the view is refused first
    assert capi.tsdf_create_raw(fake, None, C.addressof(h)) == INVALID
    assert capi.tsdf_create_raw(fake, C.addressof(plan), None) == INVALID
    for f in (L.sage_tsdf_reset,):
        f.argtypes = [C.c_void_p]
        assert f(None) == INVALID
    L.sage_tsdf_get.argtypes = [C.c_void_p] * 4
    assert L.sage_tsdf_get(None, None, None, None) == INVALID
    L.sage_tsdf_dev.argtypes = [C.c_void_p] * 4
    assert L.sage_tsdf_dev(None, None, None, None) == INVALID
    L.sage_tsdf_last_stats.argtypes = [C.c_void_p] * 2
    assert L.sage_tsdf_last_stats(None, None) == INVALID
    L.sage_tsdf_destroy.argtypes, L.sage_tsdf_destroy.restype = [C.c_void_p], None
    L.sage_tsdf_destroy(None)                                                  # a no-op

    cam = synth.Camera(30.0, 30.0, 15.5, 11.5, 32.0, 24.0)
    pose = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(np.float32)
    img = FakeTensor(24 * 32)
    good = capi.tsdf_view(img, pose, cam)

    def bad_views():
        yield "depth NULL", capi.tsdf_view(img, pose, cam)
        for field, val in (("fx", 0.0), ("fy", -2.0), ("w", 0.0), ("h", 0.0), ("fx", np.nan)):
            c2 = synth.Camera(30.0, 30.0, 15.5, 11.5, 32.0, 24.0)
            setattr(c2, field, val)
            yield f"camera {field}", capi.tsdf_view(img, pose, c2)
        p2 = pose.copy(); p2[10] = np.nan
        yield "pose", capi.tsdf_view(img, p2, cam)
        yield "obs_weight 0", capi.tsdf_view(img, pose, cam, obs_weight=0.0)
        yield "obs_weight < 0", capi.tsdf_view(img, pose, cam, obs_weight=-1.0)
        yield "std_floor < 0", capi.tsdf_view(img, pose, cam, std_floor=-0.1)
        yield "min_depth nan", capi.tsdf_view(img, pose, cam, min_depth=np.nan)
        yield "images too small", capi.tsdf_view(img, pose, cam, image_floats=24 * 32 - 1)

    assert capi.tsdf_integrate_raw(None, C.addressof(good)) == INVALID
    assert capi.tsdf_integrate_raw(fake, None) == INVALID
    for what, v in bad_views():
        if what == "depth NULL":
            v.depth_dev = None
        assert capi.tsdf_integrate_raw(fake, C.addressof(v)) == INVALID, what
        table = (capi.SageTsdfView * 2)(good, v)
        assert capi.tsdf_integrate_batch_raw(fake, C.addressof(table), 2, 0) == INVALID, what
    one = (capi.SageTsdfView * 1)(good)
    assert capi.tsdf_integrate_batch_raw(None, C.addressof(one), 1, 0) == INVALID
    assert capi.tsdf_integrate_batch_raw(fake, None, 1, 0) == INVALID
    assert capi.tsdf_integrate_batch_raw(fake, C.addressof(one), 0, 0) == INVALID
    many = (capi.SageTsdfView * 1025)(*([good] * 1025))
    assert capi.tsdf_integrate_batch_raw(fake, C.addressof(many), 1025, 0) == INVALID
    assert capi.tsdf_integrate_batch_raw(fake, C.addressof(one), 1, 1 << 8) == INVALID       # a flag that is none
    assert capi.tsdf_integrate_batch_launches(1) == capi.tsdf_integrate_batch_launches(1024) == 1
    assert capi.tsdf_integrate_batch_launches(0) == capi.tsdf_integrate_batch_launches(1025) == 0
    assert capi.tsdf_view_chunk() == 32
    kf = np.zeros(1, np.int32)
    lo, hi = C.c_float(), C.c_float()
    assert capi.window_depth_range_raw(None, kf.ctypes.data, 1, C.addressof(lo), C.addressof(hi)) == INVALID
    assert capi.window_depth_range_raw(fake, kf.ctypes.data, 1, None, C.addressof(hi)) == INVALID
    assert capi.window_fuse_tsdf_raw(None, fake, kf.ctypes.data, 1, 0, 0.0, 1.0, 1e-4) == INVALID
    assert capi.window_fuse_tsdf_raw(fake, None, kf.ctypes.data, 1, 0, 0.0, 1.0, 1e-4) == INVALID
    assert capi.window_fuse_tsdf_raw(fake, fake, kf.ctypes.data, 1, 2, 0.0, 1.0, 1e-4) == INVALID   # std_mode
