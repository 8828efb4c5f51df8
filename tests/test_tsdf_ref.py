"""The numpy restatement of TSDF fusion (tests/tsdf_ref.py), pinned by properties, and the committed cases the GPU tests
(tests/test_gpu_tsdf.py) run: the reference's kernel needs pycuda and nvcc and cannot be executed, so the oracle is the
specification restated, and what keeps the restatement honest is what a TSDF must do.  No GPU.

* Every committed case has NO ambiguous voxel (a voxel whose fp32 and fp64 decision records differ): a condition on the
  inputs, not a tolerance -- a case with one is replaced, not excused.  Every case contains what the kernel branches on:
  voxels behind the camera, off every side of the image, beyond the truncation, clipped to 1, depth and std holes; and the
  cases between them a passing voxel whose pixel coordinate lies in (-0.5, 0), which rounds to pixel 0.
* The fp32 form lies 1.8e-6 .. 6.0e-6 from the fp64 form, relative to max(1, |tsdf|), on these cases (printed by every run).
* A fronto-parallel plane seen by three views: the zero crossing of tsdf along z, interpolated, lies within half a voxel of it.
* Two views of different sigma: the crossing sits at the inverse-sigma-weighted mean depth."""
import numpy as np
import pytest

from sage_slam_amd import synth
from tests import tsdf_ref as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_committed_cases_have_no_ambiguous_voxel_and_cover_every_branch(name):
    c = R.case(name)
    scene, r32, r64 = c["scene"], c["rec32"], c["rec64"]
    amb = R.ambiguous(scene, recs32=r32, recs64=r64)
    assert int(amb.sum()) == 0, f"{int(amb.sum())} ambiguous voxels of {amb.size}: replace the case"
    W, H = int(scene["cam"].w), int(scene["cam"].h)
    front = [x["cz"] >= 1e-4 for x in r64]
    assert any((~f).any() for f in front)                                              # behind the camera
    assert any((R.roundf(x["x"])[f] < 0).any() for x, f in zip(r64, front))            # left of the image
    assert any((R.roundf(x["x"])[f] >= W).any() for x, f in zip(r64, front))           # right
    assert any((R.roundf(x["y"])[f] < 0).any() for x, f in zip(r64, front))            # above
    assert any((R.roundf(x["y"])[f] >= H).any() for x, f in zip(r64, front))           # below
    trunc = float(scene["trunc_margin"])
    inside = [f & (R.roundf(x["x"]) >= 0) & (R.roundf(x["x"]) < W) & (R.roundf(x["y"]) >= 0) & (R.roundf(x["y"]) < H)
              for x, f in zip(r64, front)]
    assert any((i & ~x["passed"] & (x["diff"] < -trunc)).any() for x, i in zip(r64, inside))   # beyond the truncation
    assert any(x["clipped"].any() for x in r64) and any((x["passed"] & ~x["clipped"]).any() for x in r64)
    assert any((v["depth"] == 0).any() for v in c["views"]) and any(((v["std"] == 0) & (v["depth"] > 0)).any() for v in c["views"])
    a = R.distance(c["vol32"]["tsdf"], c["vol64"]["tsdf"])
    print(f"tsdf restatement {name}: fp32 against fp64 {a:.3g} relative to max(1, |tsdf|); "
          f"{[int(x['passed'].sum()) for x in r64]} voxels updated per view")
    assert a < 1e-4
    assert np.array_equal(c["vol32"]["weight"], c["vol64"]["weight"].astype(np.float32))
    assert np.array_equal(c["vol32"]["color"], c["vol64"]["color"].astype(np.float32))       # integers


def test_some_case_rounds_a_negative_coordinate_to_pixel_zero():
    hits = 0
    for name in R.CASES:
        for x in R.case(name)["rec64"]:
            hits += int((x["passed"] & (((x["x"] < 0) & (x["x"] > -0.5)) | ((x["y"] < 0) & (x["y"] > -0.5)))).sum())
    assert hits > 0


def plane_scene(depths, sigmas, dims=(8, 8, 40), vs=0.05):
    """a camera at the origin of the world looking along +z at planes z = depths[i], one view each; the volume in front of it"""
    H, W = 24, 32
    cam = synth.Camera(np.float32(28.7), np.float32(28.3), np.float32(15.4), np.float32(11.6), np.float32(W), np.float32(H))
    origin = np.array([-0.5 * dims[0] * vs + 0.013, -0.5 * dims[1] * vs + 0.007, 0.4], np.float32)
    views = [dict(depth=np.full((H, W), d, np.float32), std=None if s is None else np.full((H, W), s, np.float32),
                  pose12=np.concatenate([np.eye(3).reshape(-1), [0.001 * i, -0.002 * i, 0.0]]).astype(np.float32))
             for i, (d, s) in enumerate(zip(depths, sigmas))]
    return dict(dims=dims, origin=origin, voxel_size=np.float32(vs), trunc_margin=np.float32(8 * vs), cam=cam, views=views)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_plane_zero_crossing_within_half_a_voxel(dtype):
    plane = 1.237
    scene = plane_scene([plane] * 3, [None] * 3)
    vol, recs = R.integrate(scene, dtype=dtype)
    z = float(scene["origin"][2]) + np.arange(scene["dims"][2]) * float(scene["voxel_size"])
    seen = 0
    for ix in range(scene["dims"][0]):
        for iy in range(scene["dims"][1]):
            if vol["weight"][ix, iy].max() < 3:
                continue
            zc = R.zero_crossing(vol["tsdf"][ix, iy][vol["weight"][ix, iy] > 0], z[vol["weight"][ix, iy] > 0])
            assert zc is not None and abs(zc - plane) <= 0.5 * float(scene["voxel_size"])
            seen += 1
    assert seen >= 32


def test_two_sigmas_cross_at_the_inverse_sigma_weighted_mean():
    d, s = (1.20, 1.32), (0.2, 0.6)
    scene = plane_scene(d, s)
    scene["trunc_margin"] = np.float32(1.0)                                      # nothing truncated, nothing clipped near the planes
    vol, recs = R.integrate(scene, dtype=np.float64)
    want = (d[0] / s[0] + d[1] / s[1]) / (1 / s[0] + 1 / s[1])
    z = float(scene["origin"][2]) + np.arange(scene["dims"][2]) * float(scene["voxel_size"])
    seen = 0
    for ix in range(scene["dims"][0]):
        for iy in range(scene["dims"][1]):
            full = vol["weight"][ix, iy] == 2
            if full.sum() < 8:
                continue
            zc = R.zero_crossing(vol["tsdf"][ix, iy][full], z[full])
            # (tsdf is linear in z where neither view clips: the interpolation is exact up to the fp32 inputs)
            assert zc is not None and abs(zc - want) < 1e-5, (zc, want)
            seen += 1
    assert seen >= 32
    assert abs(want - np.mean(d)) > 0.02                                         # ... and not at the plain mean
