"""numpy restatement of the tracker's overlap statistics (sage_track_overlap; CameraTracker::ComputeAreaInlierRatio,
camera_tracker.cpp:95-169): the yardstick of tests/test_overlap_host.py and tests/test_gpu_track_overlap.py.

Every function takes a ``dtype``: np.float64 is the yardstick, np.float32 rounds every intermediate to fp32 in the order the
reference's tensor expressions do -- its distance from the fp64 result is what fp32 arithmetic costs on the same inputs.
The hull is a monotone chain of its own (no code shared with the engine's), in fp64 on whatever coordinates it is given."""
import numpy as np


def hull(points):
    """convex hull of [n,2] points -> (area, corners [k,2] counter-clockwise); fp64; 0 and an empty list for fewer than three
    distinct points or a collinear set; collinear boundary points are no corners"""
    pts = sorted(set((float(x), float(y)) for x, y in np.asarray(points, np.float64).reshape(-1, 2)
                     if np.isfinite(x) and np.isfinite(y)))
    if len(pts) < 3:
        return 0.0, np.zeros((0, 2))

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and ((out[-1][0] - out[-2][0]) * (p[1] - out[-2][1])
                                     - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0])) <= 0:
                out.pop()
            out.append(p)
        return out

    lower, upper = half(pts), half(reversed(pts))
    h = np.array(lower[:-1] + upper[:-1], np.float64)
    if len(h) < 3:
        return 0.0, np.zeros((0, 2))
    x, y = h[:, 0] - h[0, 0], h[:, 1] - h[0, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)), h


def hull_area(points) -> float:
    return hull(points)[0]


def points(prob, dtype=np.float64, depth_scale=1.0):
    """per-point quantities of the problem dict (``synth.make_overlap_problem``) -> dict(x0, y0, x1, y1, z [M], pos [M] bool,
    ux, uy [M] the unnormalised tap coordinates, ix, iy [M] the tap indices as floats, tap_ok [M], inside [M] bool)"""
    T = dtype
    cam = prob["cam"]
    fx, fy, cx, cy, w, h = (T(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h))
    R, t = np.asarray(prob["R"], np.float32).astype(T), np.asarray(prob["t"], np.float32).astype(T)
    hm = np.asarray(prob["homo"], np.float32).astype(T)
    sd = (T(np.float32(depth_scale)) * np.asarray(prob["dpts0"], np.float32).astype(T)).astype(T)
    X = []
    for r in range(3):
        rh = ((R[r, 0] * hm[:, 0]).astype(T) + (R[r, 1] * hm[:, 1]).astype(T)).astype(T)
        rh = (rh + (R[r, 2] * hm[:, 2]).astype(T)).astype(T)
        X.append(((sd * rh).astype(T) + t[r]).astype(T))
    z = X[2]
    pos = z > T(prob["eps"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x1 = (((X[0] / z).astype(T) * fx).astype(T) + cx).astype(T)
        y1 = (((X[1] / z).astype(T) * fy).astype(T) + cy).astype(T)
        x0 = ((hm[:, 0] * fx).astype(T) + cx).astype(T)
        y0 = ((hm[:, 1] * fy).astype(T) + cy).astype(T)
        # grid_sample(nearest, zeros, align_corners=True) at g = 2 x / w - 1: index = nearbyint((g + 1) / 2 * (size - 1))
        gx = (((T(2) * x1).astype(T) / w).astype(T) - T(1)).astype(T)
        gy = (((T(2) * y1).astype(T) / h).astype(T) - T(1)).astype(T)
        ux = ((((gx + T(1)).astype(T) / T(2)).astype(T)) * (w - T(1))).astype(T)
        uy = ((((gy + T(1)).astype(T) / T(2)).astype(T)) * (h - T(1))).astype(T)
        ix, iy = np.rint(ux), np.rint(uy)                       # half to even
        tap_ok = (ix >= 0) & (ix <= float(w) - 1) & (iy >= 0) & (iy <= float(h) - 1)   # False for a NaN
    mask = np.asarray(prob["mask"], np.float32)
    m = np.zeros(len(z), np.float32)
    m[tap_ok] = mask[iy[tap_ok].astype(np.int64), ix[tap_ok].astype(np.int64)]
    return dict(x0=x0, y0=y0, x1=x1, y1=y1, z=z, pos=pos, ux=ux, uy=uy, ix=ix, iy=iy, tap_ok=tap_ok, inside=pos & (m > 0.5))


def stats(prob, dtype=np.float64, depth_scale=1.0):
    """the statistics of ``SageOverlapStats`` in ``dtype`` (hull areas always fp64 on the ``dtype`` coordinates)"""
    T = dtype
    p = points(prob, dtype, depth_scale)
    cam = prob["cam"]
    M = len(p["z"])
    input_area = hull_area(np.stack([p["x0"], p["y0"]], 1))
    ins = p["inside"]
    warp_area = hull_area(np.stack([p["x1"][ins], p["y1"][ins]], 1))
    pos = p["pos"]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx, dy = (p["x1"][pos] - p["x0"][pos]).astype(T), (p["y1"][pos] - p["y0"][pos]).astype(T)
        norm = np.sqrt(((dx * dx).astype(T) + (dy * dy).astype(T)).astype(T)).astype(T)
        mean = float(np.mean(norm.astype(np.float64))) if pos.any() else float("nan")
        motion = mean / float(np.sqrt(float(cam.w) ** 2 + float(cam.h) ** 2))
        area_ratio = float(np.float64(warp_area) / np.float64(input_area))      # 0 / 0: NaN, like the reference's division
    return dict(input_area=input_area, warp_area=warp_area, area_ratio=area_ratio, inlier_ratio=float(ins.sum()) / M,
                average_motion=motion, n_points=M, n_pos_depth=int(pos.sum()), n_in_mask=int(ins.sum()))


def ambiguous(prob, depth_scale=1.0):
    """[M] bool from the fp64 restatement: points whose counts fp32 may decide either way -- an unnormalised tap coordinate
    within 1e-4 px of a half-integer while within one pixel of the image, or |z - eps| < 1e-4 |z|"""
    p = points(prob, np.float64, depth_scale)
    cam = prob["cam"]
    w, h = float(cam.w), float(cam.h)
    with np.errstate(invalid="ignore"):
        def near_half(u, size):
            frac = np.abs(u - np.floor(u) - 0.5)
            return (frac < 1e-4) & (u > -1.5) & (u < size + 0.5)
        amb = near_half(p["ux"], w) | near_half(p["uy"], h) | (np.abs(p["z"] - float(prob["eps"])) < 1e-4 * np.abs(p["z"]))
    return amb


def grid_sample_taps(prob, depth_scale=1.0):
    """torch's own grid_sample (CPU) of an image whose pixel values are their raster indices + 1, at the fp32 restatement's
    (x1, y1) normalised the reference's way -> [M] int64 raster index of the tap, -1 where it reads the zero padding"""
    import torch
    import torch.nn.functional as F
    p = points(prob, np.float32, depth_scale)
    cam = prob["cam"]
    H, W = int(cam.h), int(cam.w)
    x1, y1 = torch.from_numpy(np.asarray(p["x1"], np.float32)), torch.from_numpy(np.asarray(p["y1"], np.float32))
    grid = torch.stack([2.0 * x1 / float(cam.w) - 1.0, 2.0 * y1 / float(cam.h) - 1.0], 1).reshape(1, 1, -1, 2)
    img = (torch.arange(H * W, dtype=torch.float32) + 1.0).reshape(1, 1, H, W)       # exact in fp32 up to 2^24 pixels
    out = F.grid_sample(img, grid, mode="nearest", padding_mode="zeros", align_corners=True).reshape(-1)
    return out.to(torch.int64).numpy() - 1
