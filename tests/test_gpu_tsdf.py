"""TSDF fusion on the GPU (include/sage_ba.h "TSDF fusion"): sage_tsdf_integrate against the numpy restatement of the
specification (tests/tsdf_ref.py, pinned by tests/test_tsdf_ref.py), sage_tsdf_integrate_batch against n single calls byte for
byte, the cull's statistics, the window path and misuse.

Cases (tests/tsdf_ref.CASES; test_tsdf_ref.py asserts that none has an ambiguous voxel and that each holds voxels behind the
camera, off every side of the image, beyond the truncation, depth and std holes): 24 x 20 x 28 at obs_weight 1 and 33 x 17 x 70
at obs_weight 2.5 with 5 views of 24 x 32 each -- neither is a multiple of a wave or of a brick, the z tail is ragged -- and
64 x 48 x 80 with 7 views for the batch.

Bars.
* weight (the decisions) equals the fp64 restatement exactly; color (integers) too.
* tsdf lies within 8 max(a, 2^-24) of the fp64 restatement relative to max(1, |tsdf|), a the fp32 restatement's own distance
  measured in the test (the project's bar for per-point values, tests/test_gpu_depth_scale.py).
* the device equals the fp32 restatement byte for byte: every operation of the specification is one correctly rounded fp32
  operation on the device (no contraction, IEEE division, roundf) as it is in numpy.
Every run prints a and the device's distance through conftest.summary_line."""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import tsdf_ref as R
from tests.conftest import summary_line

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, STATE = -1, -2, -4
HOLD_POSE, HOLD_CODE, HOLD_SCALE = 1, 2, 4


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def ws(capi):
    w = capi.Workspace()
    yield w
    w.close()


def volume(capi, ws, scene, color=False):
    return capi.TsdfVolume(ws, capi.tsdf_plan_exact(scene["dims"], scene["origin"], scene["voxel_size"], scene["trunc_margin"], color))


def device_views(capi, scene, views=None, color=False, std=True):
    import torch
    out = []
    for v in (scene["views"] if views is None else views):
        t = {k: torch.from_numpy(np.ascontiguousarray(v[k])).cuda() for k in ("depth", "std", "color")}
        out.append(capi.tsdf_view(t["depth"], v["pose12"], v.get("cam", scene["cam"]), std=t["std"] if std else None,
                                  color=t["color"] if color else None, obs_weight=v.get("obs_weight", 1.0),
                                  min_depth=v.get("min_depth", 1.0e-4), std_floor=v.get("std_floor", 0.0)))
    return out


def volume_bytes(vol, color=False):
    return b"".join(a.tobytes() for a in vol.get(color=color))


# ------------------------------------------------------------------------------------- 1. per image against the restatement
@pytest.mark.parametrize("name", ["24x20x28", "33x17x70"])
def test_single_views_against_the_restatement(capi, ws, name):
    c = R.case(name)
    scene = c["scene"]
    vol = volume(capi, ws, scene)
    for v in device_views(capi, scene):
        vol.integrate(v)
    tsdf, weight = vol.get()
    vol.close()
    assert np.array_equal(weight, c["vol64"]["weight"].astype(np.float32))         # the decisions, exactly
    a = R.distance(c["vol32"]["tsdf"], c["vol64"]["tsdf"])
    dev = R.distance(tsdf, c["vol64"]["tsdf"])
    same = tsdf.tobytes() == c["vol32"]["tsdf"].tobytes()
    summary_line(f"tsdf integrate {name}: fp32 restatement {a:.3g}, device {dev:.3g} from fp64 (relative to max(1, |tsdf|)); "
                 f"device == fp32 restatement byte for byte: {same}; {int((weight > 0).sum())} of {weight.size} voxels touched")
    assert dev <= 8 * max(a, 2.0 ** -24)
    assert same


# ------------------------------------------------------------------------------------------------------------ 2. color
def test_color_channels_equal_the_restatement(capi, ws):
    c = R.case("24x20x28")
    scene = c["scene"]
    vol = volume(capi, ws, scene, color=True)
    for v in device_views(capi, scene, color=True):
        vol.integrate(v)
    tsdf, weight, color = vol.get(color=True)
    vol.close()
    want = c["vol64"]["color"]
    assert np.array_equal(color, want.astype(np.float32))                          # integers: every channel exactly
    assert np.unique(color).size > 100 and color.max() < 2 ** 24
    assert tsdf.tobytes() == c["vol32"]["tsdf"].tobytes() and np.array_equal(weight, c["vol32"]["weight"])


# ------------------------------------------------------------------------------------------ 3. batch == singles, byte for byte
@pytest.mark.parametrize("n", [1, 2, 7, 33])
@pytest.mark.parametrize("name", ["24x20x28", "33x17x70", "64x48x80"])
def test_batch_equals_singles_byte_for_byte(capi, ws, name, n):
    assert 33 == capi.tsdf_view_chunk() + 1                                        # one more than the LDS chunk
    scene = R.case(name, n=n + 2)["scene"]
    views = device_views(capi, scene, color=True)
    single, batch = volume(capi, ws, scene, color=True), volume(capi, ws, scene, color=True)
    for v in views[:2]:                                                            # the volume already holds earlier views
        single.integrate(v)
    start = single.get(color=True)
    for v in views[2:]:
        single.integrate(v)
    want = volume_bytes(single, color=True)
    assert want != b"".join(a.tobytes() for a in start)
    flags = [0, capi.TSDF_NO_CULL, 0, capi.TSDF_BRICK_X1, capi.TSDF_BRICK_X2 | capi.TSDF_NO_CULL, capi.TSDF_BRICK_X4]
    for fl in flags:                                                               # (flags 0 twice: two runs, identical bytes)
        batch.reset()
        batch.integrate_batch(views[:2])
        batch.integrate_batch(views[2:], flags=fl)
        assert volume_bytes(batch, color=True) == want, (name, n, fl)
    assert capi.tsdf_integrate_batch_launches(n) == 1
    single.close(); batch.close()


# -------------------------------------------------------------------------------------------------------- 4. cull statistics
def test_cull_statistics(capi, ws):
    scene = R.case("64x48x80")["scene"]
    views = device_views(capi, scene)
    vol = volume(capi, ws, scene)
    vol.integrate_batch(views)
    st = vol.last_stats()
    assert st.views == len(views) and st.pairs == st.bricks * len(views) and list(st.brick) == [4, 4, 64]
    assert st.bricks == 16 * 12 * 2 and 0 < st.pairs_kept < st.pairs
    kept = st.pairs_kept
    before = volume_bytes(vol)
    vol.integrate_batch(views, flags=capi.TSDF_NO_CULL)
    st = vol.last_stats()
    assert st.pairs_kept == st.pairs
    summary_line(f"tsdf cull 64x48x80, 7 views: {kept} of {st.pairs} brick-view pairs kept ({kept / st.pairs:.2f})")
    # a view entirely outside the volume: the camera beyond the volume, looking away from it
    away = dict(scene["views"][0])
    centre = scene["origin"].astype(np.float64) + 0.5 * np.array(scene["dims"]) * float(scene["voxel_size"])
    R0 = synth.so3_exp(np.array([0.3, -0.2, 0.1]))
    away["pose12"] = np.concatenate([R0.reshape(-1), centre + R0[:, 2] * 5.0]).astype(np.float32)   # z axis points away
    before = volume_bytes(vol)
    vol.integrate_batch(device_views(capi, scene, [away]))
    st = vol.last_stats()
    assert st.pairs_kept == 0 and st.pairs == st.bricks
    assert volume_bytes(vol) == before
    vol.close()


# ------------------------------------------------------------------------------------------------------------- 5. the window
def test_window_fuse_and_depth_range(capi, ws):
    import torch
    K, CS, H, W = 3, 16, 24, 32
    w = synth.make_window(K=K, H=H, W=W, FS=16, CS=CS, L=2, n_samples=300, seed=41, back_links=3)
    dks = [capi.DeviceKeyframe(kf, H, W) for kf in w.keyframes]
    prepared = {1: capi.PreparedKeyframe.prepare_batch(ws, capi.prepare_config(w), [dks[1]])[0]}
    win = capi.Window(w, holds={2: HOLD_CODE | HOLD_SCALE}, prepared=prepared)
    st = capi.SageLmState(); st.damp = 1e-3
    cfg = capi.lm_config_default(); cfg.max_inner_evals = 1
    win.lm_step(st, cfg)                                                           # move the variables off their initial values
    win.linearize()
    kfs = [2, 0, 1]
    maps, poses = [], []
    for k in kfs:
        pose, code, scale = win.get_keyframe(k)
        maps.append(capi.depth_and_grad(ws, win.kfs[k].bias, win.kfs[k].basis, code, scale, H, W, CS)[0])
        poses.append(pose)
    torch.cuda.synchronize()
    # the depth range, exactly
    mask = win.mask.cpu().numpy().reshape(H, W)
    host = np.stack([np.where(mask <= 0.5, np.float32(0), m.cpu().numpy()) for m in maps])
    lo, hi = capi.window_depth_range(win, kfs)
    assert lo == host[host > 0].min() and hi == host.max() and 0 < lo < hi
    assert capi.window_depth_range(win, [K], check=False)[0] == INVALID
    # a volume over the three frusta
    cam = w.cams[0]
    bounds = np.array([np.inf] * 3 + [-np.inf] * 3)
    for p in poses:
        bounds = capi.tsdf_frustum_bounds(cam, p, hi, bounds)
    plan = capi.tsdf_plan(bounds, 0.1, 3.0e4, 4.0)
    vol, ref = capi.TsdfVolume(ws, plan), capi.TsdfVolume(ws, plan)
    assert capi.window_fuse_tsdf(win, vol, kfs, capi.TSDF_STD_SIGMA, check=False) == STATE      # no Sigma yet
    assert not np.any(vol.get()[1])
    win.solve(0.0)
    win.covariance()

    def batch(std=None, floor=0.0, ow=1.0):
        ref.reset()
        ref.integrate_batch([capi.tsdf_view(m.reshape(-1), p, cam, std=None if std is None else std[i], mask=win.mask.reshape(-1),
                                            obs_weight=ow, min_depth=1e-3, std_floor=floor)
                             for i, (m, p) in enumerate(zip(maps, poses))])
        return volume_bytes(ref)

    capi.window_fuse_tsdf(win, vol, kfs, capi.TSDF_STD_ONE, 0.0, 1.5, 1e-3)
    assert volume_bytes(vol) == batch(ow=1.5) and np.any(vol.get()[1])
    sig = win.depth_sigma(kfs)
    torch.cuda.synchronize()
    assert not sig[0].any() and sig[1].min() > 0                                   # keyframe 2 is held: its sigma map is 0
    vol.reset()
    capi.window_fuse_tsdf(win, vol, kfs, capi.TSDF_STD_SIGMA, 0.0, 1.0, 1e-3)
    assert volume_bytes(vol) == batch(std=[s.reshape(-1) for s in sig])
    two = vol.get()[1]
    vol.reset()
    capi.window_fuse_tsdf(win, vol, kfs[1:], capi.TSDF_STD_SIGMA, 0.0, 1.0, 1e-3)
    assert np.array_equal(vol.get()[1], two)                                       # the held keyframe contributed nothing ...
    vol.reset()
    capi.window_fuse_tsdf(win, vol, kfs, capi.TSDF_STD_SIGMA, 0.05, 1.0, 1e-3)
    assert volume_bytes(vol) == batch(std=[s.reshape(-1) for s in sig], floor=0.05)
    assert vol.get()[1].sum() > two.sum()                                          # ... and contributes with a positive floor
    summary_line(f"window fuse K 3 24x32: volume {tuple(plan.dim)}, {int((two > 0).sum())} voxels touched by two keyframes, "
                 f"{int((vol.get()[1] > 0).sum())} by three (std_floor 0.05); depth range [{lo:.3g}, {hi:.3g}]")
    # misuse: a status code, the volume unchanged
    before = volume_bytes(vol)
    assert capi.window_fuse_tsdf(win, vol, [0, K], check=False) == INVALID
    assert capi.window_fuse_tsdf(win, vol, [], check=False) == INVALID
    assert capi.window_fuse_tsdf(win, vol, [0], obs_weight=0.0, check=False) == INVALID
    assert capi.window_fuse_tsdf(win, None, [0], check=False) == INVALID
    win.close()
    assert capi.window_fuse_tsdf(win, vol, [0], check=False) == INVALID            # a destroyed window
    assert volume_bytes(vol) == before
    vol.close(); ref.close()
    prepared[1].release()


# ----------------------------------------------------------------------------------------------------- 6. misuse on the device
def test_misuse_leaves_the_volume_unchanged(capi, ws):
    scene = R.case("24x20x28")["scene"]
    vol = volume(capi, ws, scene)                                                  # (no color volume)
    views = device_views(capi, scene, color=True)
    plain = device_views(capi, scene)
    vol.integrate(plain[0])
    before = volume_bytes(vol)
    assert vol.integrate(views[1], check=False) == INVALID                         # a color image, no color volume
    assert vol.integrate_batch([plain[1], views[2]], check=False) == INVALID
    v = device_views(capi, scene)[1]
    v.depth_dev = None
    assert vol.integrate(v, check=False) == INVALID and vol.integrate_batch([plain[1], v], check=False) == INVALID
    v = device_views(capi, scene)[1]
    v.image_floats = 24 * 32 - 1                                                   # images smaller than the camera says
    assert vol.integrate(v, check=False) == INVALID and vol.integrate_batch([v], check=False) == INVALID
    v = device_views(capi, scene)[1]
    v.obs_weight = 0.0
    assert vol.integrate(v, check=False) == INVALID
    assert vol.integrate_batch([], check=False) == INVALID
    assert vol.integrate_batch([plain[1]], flags=1 << 9, check=False) == INVALID
    assert volume_bytes(vol) == before
    vol.integrate_batch([plain[1]])                                                # ... and it still works
    assert volume_bytes(vol) != before
    vol.close()
