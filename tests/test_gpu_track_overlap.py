"""sage_track_overlap (CameraTracker::ComputeAreaInlierRatio on the device, the hulls of the surviving points on the host)
against the fp64 restatement of tests/overlap_ref.py.

Inputs: synth.make_overlap_problem at 48x64 (M = 2176: 9 workgroups, one grid pass) and one case at 96x128 (M = 8708: more
points than the 32 workgroups of one grid pass hold).  The seeds are those at which the fp64 restatement finds no ambiguous
point (a tap coordinate within 1e-4 px of a half-integer, or a depth within 1e-4 of eps), so the counts are exact.

Bounds.  Areas, area ratio and motion are compared with the fp64 restatement; a quantity may be off by 8 x the larger of
(a) the relative distance of the fp32 restatement from the fp64 one on the same inputs, measured by the test on the CPU, and
(b) 2^-24.  Measured (a) and the bound it gives:

  case (size, seed)      area_ratio  -> bound      input / warp area        motion   -> bound
  small  (48x64, 1)      1.2e-8      -> 4.8e-7     5.9e-9 / 1.7e-8          7.5e-8   -> 6.0e-7
  big    (48x64, 0)      8.2e-8      -> 6.5e-7     5.9e-9 / 8.8e-8          8.7e-9   -> 4.8e-7
  big96  (96x128, 1)     2.8e-8      -> 4.8e-7     1.4e-8 / 4.2e-8          9.9e-9   -> 4.8e-7
  behind (48x64, 2)      (no in-mask point: warp_area == 0, area_ratio == 0)         4.7e-7   -> 3.8e-6

What the device gave on an MI355X (relative distance from fp64): area_ratio 1.0e-8 / 1.2e-7 / 5.0e-8 (small / big / big96), motion
1.1e-7 / 3.7e-8 / 2.3e-8, behind's motion 4.5e-7; both areas equal the host hull over all points of the set exactly.

In "behind" the motion is carried by the points whose depth is close to eps (coordinates of 1e4 px and more): its bound is
measured for that case on its own, by the same rule."""
import functools

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import overlap_ref as ref

pytestmark = pytest.mark.gpu

CASES = {"small": (48, 64, "small", 1), "big": (48, 64, "big", 0), "behind": (48, 64, "behind", 2), "big96": (96, 128, "big", 1)}
EPS24 = 2.0 ** -24


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


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, fp64 statistics, fp32 statistics, fp32 points, number of ambiguous points): computed once, never changed"""
    H, W, pose, seed = CASES[name]
    rot, tr = synth.OVERLAP_POSES[pose]
    prob = synth.make_overlap_problem(H, W, rot, tr, seed)
    return prob, ref.stats(prob, np.float64), ref.stats(prob, np.float32), ref.points(prob, np.float32), int(ref.ambiguous(prob).sum())


def run(capi, ws, prob, depth_scale=1.0, **over):
    import torch
    p = {**prob, **over}
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    return capi.track_overlap(ws, p["R"], p["t"], dv(p["dpts0"]), dv(p["homo"]), p["cam"], dv(p["mask"]), p["eps"], depth_scale)


def raw(st):
    return bytes(memoryview(st))


def bound(v32, v64):
    """8 x the larger of the fp32 restatement's relative distance from the fp64 one and 2^-24"""
    return 8.0 * max(abs(v32 - v64) / abs(v64), EPS24)


def close(got, want, rel, what):
    d = abs(got - want) / abs(want)
    print(f"    {what}: got {got!r} want {want!r} rel {d:.2e} bound {rel:.2e}")
    return d <= rel


@pytest.mark.parametrize("name", list(CASES))
def test_statistics_match_the_fp64_restatement(capi, ws, name):
    prob, s64, s32, p32, n_amb = case(name)
    st = run(capi, ws, prob)
    M = prob["M"]
    print(f"{name}: M {M} ambiguous {n_amb}  pos {st.n_pos_depth}/{s64['n_pos_depth']}  in {st.n_in_mask}/{s64['n_in_mask']}  "
          f"candidates {list(st.n_candidates)}")
    assert st.n_points == M
    assert n_amb <= 0.005 * M
    assert abs(st.n_pos_depth - s64["n_pos_depth"]) <= n_amb and abs(st.n_in_mask - s64["n_in_mask"]) <= n_amb
    assert st.inlier_ratio == np.float32(st.n_in_mask) / np.float32(M)
    assert close(st.input_area, s64["input_area"], bound(s32["input_area"], s64["input_area"]), "input_area")
    if s64["n_in_mask"] == 0:                   # "behind": nothing lands in the mask
        assert st.n_in_mask == 0 and st.warp_area == 0.0 and st.area_ratio == 0.0 and st.n_candidates[1] == 0
        assert 0 < s64["n_pos_depth"] < M       # ... but a part of the points keeps a positive depth
    else:
        assert close(st.warp_area, s64["warp_area"], bound(s32["warp_area"], s64["warp_area"]), "warp_area")
        assert close(st.area_ratio, s64["area_ratio"], bound(s32["area_ratio"], s64["area_ratio"]), "area_ratio")
    assert close(st.average_motion, s64["average_motion"], bound(s32["average_motion"], s64["average_motion"]), "average_motion")


@pytest.mark.parametrize("name", list(CASES))
def test_the_filter_drops_no_hull_vertex(capi, ws, name):
    """the two areas equal sage_convex_hull_area over ALL points of the set (the fp32 restatement's coordinates), to the
    bound of the areas above; the device handed over some points of a non-empty set and never more than it has"""
    prob, s64, s32, p32, _ = case(name)
    st = run(capi, ws, prob)
    all0, _ = capi.convex_hull_area(np.stack([p32["x0"], p32["y0"]], 1))
    ins = p32["inside"]
    all1, _ = capi.convex_hull_area(np.stack([p32["x1"][ins], p32["y1"][ins]], 1))
    print(f"{name}: candidates {list(st.n_candidates)} of {prob['M']} / {int(ins.sum())}")
    assert close(st.input_area, all0, bound(s32["input_area"], s64["input_area"]), "input_area vs hull of all points")
    assert 0 < st.n_candidates[0] <= prob["M"]
    if ins.any():
        assert close(st.warp_area, all1, bound(s32["warp_area"], s64["warp_area"]), "warp_area vs hull of all points")
        assert 0 < st.n_candidates[1] <= int(ins.sum())
    else:
        assert st.warp_area == all1 == 0.0 and st.n_candidates[1] == 0


def circle_problem():
    """360 source pixels on a circle of radius 100 px about the centre of a 320x256 camera, identity pose, mask all ones"""
    cam = synth.Camera(*[np.float32(v) for v in (288.0, 288.0, 159.5, 127.5, 320.0, 256.0)])
    a = 2.0 * np.pi * np.arange(360) / 360
    x, y = 159.5 + 100.0 * np.cos(a), 127.5 + 100.0 * np.sin(a)
    homo = np.stack([(x - 159.5) / 288.0, (y - 127.5) / 288.0, np.ones(360)], 1).astype(np.float32)
    return dict(cam=cam, mask=np.ones((256, 320), np.float32), dpts0=np.ones(360, np.float32), homo=homo,
                R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), eps=np.float32(1e-4), M=360)


def test_a_set_that_is_all_hull_survives_whole(capi, ws):
    """every point of a circle is a hull vertex: none may be dropped (neighbours are 1.7 px apart and 0.015 px off the chord
    of their neighbours, a thousand times the rounding of a coordinate).  The area: the hull of the fp32 restatement's points
    to 8 x 2^-24, and the closed form 1/2 r^2 n sin(2 pi / n) to 1e-6 -- a coordinate h * fx + cx carries three fp32 roundings
    at sizes <= 260, a corner is off by <= 4e-5 px, the area by <= 2 d / r = 8e-7 of it"""
    prob = circle_problem()
    st = run(capi, ws, prob)
    p32 = ref.points(prob, np.float32)
    want, corners = ref.hull(np.stack([p32["x0"], p32["y0"]], 1))
    print(f"circle: candidates {list(st.n_candidates)} in {st.n_in_mask}")
    assert len(corners) == 360
    assert st.n_candidates[0] == 360
    assert close(st.input_area, want, 8 * EPS24, "input_area vs fp64 hull of the fp32 points")
    assert close(st.input_area, 0.5 * 100.0 ** 2 * 360 * np.sin(2 * np.pi / 360), 1e-6, "input_area vs closed form")
    assert st.n_in_mask == st.n_pos_depth == 360 and st.n_candidates[1] == 360      # the warped set is the same circle
    assert close(st.warp_area, want, 1e-6, "warp_area")
    assert st.average_motion < 1e-6


def test_mask_all_zero(capi, ws):
    prob, s64, _, _, _ = case("small")
    st = run(capi, ws, prob, mask=np.zeros_like(prob["mask"]))
    assert st.n_in_mask == 0 and st.warp_area == 0.0 and st.inlier_ratio == 0.0 and st.area_ratio == 0.0
    assert st.n_candidates[1] == 0 and st.n_pos_depth == s64["n_pos_depth"]
    assert np.isfinite(st.average_motion) and st.average_motion > 0


def test_eps_above_every_depth(capi, ws):
    prob, s64, s32, _, _ = case("small")
    st = run(capi, ws, prob, eps=np.float32(1e6))
    assert st.n_pos_depth == 0 and st.n_in_mask == 0 and np.isnan(st.average_motion)
    assert st.warp_area == 0.0 and st.area_ratio == 0.0
    assert close(st.input_area, s64["input_area"], bound(s32["input_area"], s64["input_area"]), "input_area")


@pytest.mark.parametrize("M", [1, 2])
def test_one_and_two_points(capi, ws, M):
    prob, _, _, _, _ = case("small")
    mid = prob["M"] // 2                                   # points in the middle of the image: they land inside the mask
    sub = {**prob, "dpts0": prob["dpts0"][mid:mid + M], "homo": prob["homo"][mid:mid + M], "M": M}
    s64, s32 = ref.stats(sub, np.float64), ref.stats(sub, np.float32)
    st = run(capi, ws, sub)
    assert (st.n_points, st.n_pos_depth, st.n_in_mask) == (M, s64["n_pos_depth"], s64["n_in_mask"]) == (M, M, M)
    assert st.input_area == 0.0 and st.warp_area == 0.0 and np.isnan(st.area_ratio) and st.inlier_ratio == 1.0
    assert list(st.n_candidates) == [M, M]
    assert close(st.average_motion, s64["average_motion"], bound(s32["average_motion"], s64["average_motion"]), "average_motion")


def test_all_points_on_one_image_row(capi, ws):
    """identity rotation, unit depths: source and warped points share one image row -- both areas 0, area_ratio = 0 / 0 = NaN"""
    cam = synth.Camera(*[np.float32(v) for v in (57.6, 57.6, 31.5, 23.5, 64.0, 48.0)])
    x = np.arange(4, 60, dtype=np.float32)
    homo = np.stack([(x - cam.cx) / cam.fx, np.full_like(x, (20.0 - 23.5) / 57.6), np.ones_like(x)], 1).astype(np.float32)
    prob = dict(cam=cam, mask=np.ones((48, 64), np.float32), dpts0=np.ones(len(x), np.float32), homo=homo,
                R=np.eye(3, dtype=np.float32), t=np.array([0.01, 0.0, 0.0], np.float32), eps=np.float32(1e-4), M=len(x))
    st = run(capi, ws, prob)
    assert st.n_in_mask == len(x) and st.input_area == 0.0 and st.warp_area == 0.0 and np.isnan(st.area_ratio)
    assert st.inlier_ratio == 1.0 and np.isfinite(st.average_motion)


def test_depth_scale_multiplies_the_depths_first(capi, ws):
    """depth_scale = s on the depths d is depth_scale = 1 on fp32(s * d): bit for bit"""
    prob, _, _, _, _ = case("small")
    s = np.float32(1.37)
    a = run(capi, ws, prob, depth_scale=float(s))
    b = run(capi, ws, prob, dpts0=(s * prob["dpts0"]).astype(np.float32))
    one = run(capi, ws, prob)
    assert raw(a) == raw(b)
    assert raw(a) != raw(one)                              # ... and the scale does change the result


@pytest.mark.parametrize("name", ["small", "big96"])
def test_two_calls_return_the_same_bytes(capi, ws, name):
    """sums over per-workgroup partials in a fixed order and a host hull that sorts its input: nothing of the order in which
    the survivors were appended reaches the result -- n_candidates included, the set of survivors is a function of the inputs"""
    prob, _, _, _, _ = case(name)
    a, b = run(capi, ws, prob), run(capi, ws, prob)
    assert raw(a) == raw(b)
    w2 = capi.Workspace()                                  # a fresh workspace (fresh buffers) too
    try:
        assert raw(run(capi, w2, prob)) == raw(a)
    finally:
        w2.close()


def test_tracker_and_overlap_share_a_workspace(capi, orc):
    """sage_track_frame, sage_track_overlap, sage_track_frame on ONE workspace: the ticket and the pinned regions are shared
    without colliding -- both tracker results are identical, and the overlap statistics equal those of a workspace of their own"""
    from tests.test_gpu_tracker import Scene
    scene = Scene(capi, orc)
    try:
        cfg = capi.lm_config_default()
        cfg.max_num_iters = 3
        tprob = scene.problem(6, True, False)
        prob, _, _, _, _ = case("small")
        first = capi.track_frame(cfg, 6, tprob, scene.start_pose(), 1.0)
        st = run(capi, scene.ws, prob)
        second = capi.track_frame(cfg, 6, tprob, scene.start_pose(), 1.0)
        assert first[0] == 0 and second[0] == 0
        assert first[1].tobytes() == second[1].tobytes() and first[2:] == second[2:]
        own = capi.Workspace()
        try:
            assert raw(run(capi, own, prob)) == raw(st)
        finally:
            own.close()
    finally:
        scene.close()
