"""CPU tests of the overlap statistics' host side (no GPU): sage_convex_hull_area against the fp64 hull of
tests/overlap_ref.py and against closed forms, the fp32 restatement's mask taps against torch's own grid_sample (what the
device kernel is held to in tests/test_gpu_track_overlap.py), and the argument checks of sage_track_overlap that need no
device."""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import capi, synth
from tests import overlap_ref as ref


def circle(n, r, cx=0.0, cy=0.0):
    a = 2.0 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1).astype(np.float32)


SQUARE = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 0.5], [0.25, 0.75], [1, 1], [0, 0], [0.5, 0.0], [0.9, 0.1]], np.float32)


def hull_cases():
    rng = np.random.default_rng(5)
    return {
        "square_interior_duplicates": SQUARE,
        "triangle": np.array([[3, 1], [7, 2], [4, 6]], np.float32),
        "collinear": np.stack([np.arange(9.0), 2.0 * np.arange(9.0) + 1.0], 1).astype(np.float32),
        "circle360": circle(360, 100.0, 160.0, 128.0),
        "cloud": rng.normal(0.0, 50.0, (500, 2)).astype(np.float32),
        "far_from_origin": (rng.random((200, 2)) + 4000.0).astype(np.float32),
    }


@pytest.mark.parametrize("name", list(hull_cases()))
def test_hull_area_matches_the_fp64_reference_hull(name):
    """both hulls run in fp64 on the same fp32-valued points; their corner sets agree, so the areas differ only by the
    rounding of a sum of at most a few hundred exact products: 1e-12 relative is three orders above that"""
    pts = hull_cases()[name]
    area, nv = capi.convex_hull_area(pts)
    want, corners = ref.hull(pts)
    assert nv == len(corners)
    assert area == pytest.approx(want, rel=1e-12, abs=0.0)


def test_hull_area_closed_forms():
    area, nv = capi.convex_hull_area(SQUARE)
    assert area == 1.0 and nv == 4
    area, nv = capi.convex_hull_area(hull_cases()["triangle"])
    assert area == 0.5 * abs((7 - 3) * (6 - 1) - (2 - 1) * (4 - 3)) and nv == 3
    area, nv = capi.convex_hull_area(hull_cases()["collinear"])
    assert area == 0.0 and nv == 0


def test_hull_area_of_a_circle_keeps_every_point():
    """360 points on a circle of radius 100: every one is a corner; the area is 1/2 r^2 n sin(2 pi / n) up to the fp32
    rounding of the coordinates -- each is off by at most half a spacing of fp32 at its size (<= 260: 1.5e-5 px), a corner
    by at most d = 2.2e-5 px; moving every corner outwards by d changes the area by perimeter * d, 2 d / r = 4.4e-7 of it at
    the very worst (the signs are mixed: the measured distance is ~1e-8)"""
    r, n = 100.0, 360
    area, nv = capi.convex_hull_area(circle(n, r, 160.0, 128.0))
    assert nv == n
    want = 0.5 * r * r * n * np.sin(2.0 * np.pi / n)
    print(f"circle: area {area!r} closed form {want!r} rel {abs(area - want) / want:.2e}")
    assert area == pytest.approx(want, rel=4.4e-7)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_hull_area_of_fewer_than_three_points_is_zero(n):
    pts = np.array([[1, 2], [3, 5]], np.float32)[:n]
    area = C.c_double(-1.0); nv = C.c_int(-1)
    rc = capi.lib().sage_convex_hull_area(capi._fp(np.ascontiguousarray(pts)) if n else None, n, C.byref(area), C.byref(nv))
    assert rc == 0 and area.value == 0.0 and nv.value == 0
    # three points, two of them the same
    assert capi.convex_hull_area(np.array([[1, 2], [3, 5], [1, 2]], np.float32)) == (0.0, 0)


def test_hull_area_rejects_bad_arguments():
    L = capi.lib()
    pts = np.zeros((3, 2), np.float32)
    area = C.c_double()
    assert L.sage_convex_hull_area(capi._fp(pts), 3, None, None) == -1
    assert L.sage_convex_hull_area(capi._fp(pts), -1, C.byref(area), None) == -1
    assert L.sage_convex_hull_area(None, 3, C.byref(area), None) == -1
    assert L.sage_convex_hull_area(capi._fp(pts), 3, C.byref(area), None) == 0       # n_vertices is optional


@pytest.mark.parametrize("name", list(hull_cases()))
def test_hull_area_ignores_the_order_of_the_points(name):
    pts = hull_cases()[name]
    first = capi.convex_hull_area(pts)
    rng = np.random.default_rng(11)
    for _ in range(3):
        assert capi.convex_hull_area(pts[rng.permutation(len(pts))]) == first         # the identical double


def test_hull_area_leaves_out_non_finite_points():
    pts = np.concatenate([SQUARE, np.array([[np.nan, 0.5], [0.5, np.inf]], np.float32)])
    assert capi.convex_hull_area(pts) == (1.0, 4)


@pytest.mark.parametrize("pose", list(synth.OVERLAP_POSES))
@pytest.mark.parametrize("size", [(48, 64), (96, 128)])
def test_restated_mask_taps_are_grid_samples(pose, size):
    """the tap of the fp32 restatement -- nearbyint(((2 x / w - 1) + 1) / 2 (w - 1)), half to even, zero outside -- is the
    pixel torch.nn.functional.grid_sample(nearest, zeros, align_corners=True) reads, point by point"""
    rot, tr = synth.OVERLAP_POSES[pose]
    prob = synth.make_overlap_problem(size[0], size[1], rot, tr, seed=0)
    p = ref.points(prob, np.float32)
    mine = np.where(p["tap_ok"], p["iy"] * size[1] + p["ix"], -1).astype(np.int64)
    taps = ref.grid_sample_taps(prob)
    assert np.array_equal(mine, taps)
    if pose != "behind":
        assert (taps >= 0).sum() > 0.15 * prob["M"] and (taps < 0).sum() > 0            # both branches are exercised


def test_generator_reproduces_the_prototype_sizes():
    assert synth.make_overlap_problem(48, 64)["M"] == 2176
    a, b = synth.make_overlap_problem(48, 64, seed=3), synth.make_overlap_problem(48, 64, seed=3)
    assert all(np.array_equal(a[k], b[k]) for k in ("mask", "dpts0", "homo", "R", "t"))


def test_track_overlap_checks_its_arguments_before_touching_the_device():
    """NULL pointers, M <= 0 and a bad camera answer SAGE_E_INVALID without a launch: the workspace and the device pointers
    here are not real (nothing may dereference them)"""
    fake = C.create_string_buffer(64)
    ws = C.addressof(fake)
    R = np.eye(3, dtype=np.float32).reshape(9); t = np.zeros(3, np.float32)
    cam = capi.SageCamera(57.6, 57.6, 31.5, 23.5, 64.0, 48.0)
    out = capi.SageOverlapStats()
    good = dict(ws=ws, R=R.ctypes.data, t=t.ctypes.data, dpts0=ws, depth_scale=1.0, homo=ws, M=16, cam=C.addressof(cam), mask=ws,
                eps=1e-4, out=C.addressof(out))
    call = lambda **kw: capi.track_overlap_raw(*[{**good, **kw}[k] for k in ("ws", "R", "t", "dpts0", "depth_scale", "homo", "M",
                                                                              "cam", "mask", "eps", "out")])
    for name in ("ws", "R", "t", "dpts0", "homo", "cam", "mask", "out"):
        assert call(**{name: None}) == -1, name
    assert call(M=0) == -1 and call(M=-5) == -1
    for field, bad in (("fx", 0.0), ("fx", -1.0), ("fx", float("nan")), ("fy", float("inf")), ("fy", 0.0), ("w", 0.5), ("h", 0.0),
                       ("w", float("nan"))):
        c2 = capi.SageCamera(57.6, 57.6, 31.5, 23.5, 64.0, 48.0)
        setattr(c2, field, bad)
        assert call(cam=C.addressof(c2)) == -1, (field, bad)
