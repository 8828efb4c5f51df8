"""numpy restatement of the mapper's depth-scale correction (sage_depth_scale_ratio; Mapper::CorrectDepthScale,
mapper.cpp:237-309, and df::CorrectDepthScale, mapping_utils.h:797-865) and of torch::median's lower median
(sage_median_f32): the yardstick of tests/test_depth_scale_ref.py, tests/test_gpu_depth_scale.py and tests/test_gpu_median.py.

Every function takes a ``dtype``: np.float64 is the yardstick, np.float32 rounds every intermediate to fp32 in the order the
reference's tensor expressions do -- its distance from the fp64 result is what fp32 arithmetic costs on the same inputs."""
import numpy as np


def lower_median(values, drop_nan=False):
    """torch::median of a 1-D array -> (median, n_used, n_nan): element (n_used - 1) // 2 of the sorted values; NaN when a NaN
    is present and not ``drop_nan``, and of no value at all.  The dtype of ``values`` is kept."""
    v = np.asarray(values).reshape(-1)
    nan = np.isnan(v)
    n_nan = int(nan.sum())
    n_used = int(v.size) - n_nan if drop_nan else int(v.size)
    if v.size - n_nan == 0 or (n_nan and not drop_nan):
        return v.dtype.type(np.nan), n_used, n_nan
    kept = np.sort(v[~nan])
    return kept[(kept.size - 1) // 2], n_used, n_nan


def _tap(img, jy, jx, ok):
    out = np.zeros(jx.shape, img.dtype)
    out[ok] = img[jy[ok].astype(np.int64), jx[ok].astype(np.int64)]
    return out


def bilinear_zeros(img, ix, iy, T):
    """grid_sample(bilinear, zeros) of img [H,W] at the un-normalised coordinates: weights from floor, the taps summed in the
    order nw, ne, sw, se; an in-bounds tap is multiplied in whatever its weight; a tap outside (or a non-finite coordinate)
    adds nothing"""
    H, W = img.shape
    img = img.astype(T)
    with np.errstate(invalid="ignore", over="ignore"):
        x0, y0 = np.floor(ix), np.floor(iy)
        x1, y1 = (x0 + T(1)).astype(T), (y0 + T(1)).astype(T)
        wx1, wx0 = (x1 - ix).astype(T), (ix - x0).astype(T)
        wy1, wy0 = (y1 - iy).astype(T), (iy - y0).astype(T)
        inx0, inx1 = (x0 >= 0) & (x0 <= W - 1), (x1 >= 0) & (x1 <= W - 1)      # False for a NaN
        iny0, iny1 = (y0 >= 0) & (y0 <= H - 1), (y1 >= 0) & (y1 <= H - 1)
        out = np.zeros(ix.shape, T)
        for (jy, jx, ok, w) in ((y0, x0, inx0 & iny0, (wx1 * wy1).astype(T)), (y0, x1, inx1 & iny0, (wx0 * wy1).astype(T)),
                                (y1, x0, inx0 & iny1, (wx1 * wy0).astype(T)), (y1, x1, inx1 & iny1, (wx0 * wy0).astype(T))):
            term = (_tap(img, jy, jx, ok) * w).astype(T)
            out = np.where(ok, (out + term).astype(T), out)
    return out


def points(prob, dtype=np.float64):
    """per-point quantities of the problem dict (``synth.make_depth_scale_problem``) -> dict(z [M], pos [M] bool, ix, iy [M] the
    un-normalised sampling coordinates, D1 [M], m [M], valid [M], selected [M] bool, ratio [M])"""
    T = dtype
    cam = prob["cam"]
    fx, fy, cx, cy, w, h = (T(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h))
    H, W = int(cam.h), int(cam.w)
    R, t = np.asarray(prob["R"], np.float32).astype(T), np.asarray(prob["t"], np.float32).astype(T)
    hm = np.asarray(prob["homo"], np.float32).astype(T)
    d0 = np.asarray(prob["dpts0"], np.float32).astype(T)
    X = []
    for r in range(3):
        rh = ((R[r, 0] * hm[:, 0]).astype(T) + (R[r, 1] * hm[:, 1]).astype(T)).astype(T)
        rh = (rh + (R[r, 2] * hm[:, 2]).astype(T)).astype(T)
        X.append(((d0 * rh).astype(T) + t[r]).astype(T))
    z = X[2]
    pos = z > T(prob["eps"])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = (((X[0] / z).astype(T) * fx).astype(T) + cx).astype(T)
        y = (((X[1] / z).astype(T) * fy).astype(T) + cy).astype(T)
        gx = (((x + T(0.5)).astype(T) * (T(2) / w)).astype(T) - T(1)).astype(T)
        gy = (((y + T(0.5)).astype(T) * (T(2) / h)).astype(T) - T(1)).astype(T)
        # grid_sample's un-normalisation, align_corners = false
        ix = ((((gx + T(1)).astype(T) * T(W)).astype(T) - T(1)).astype(T) / T(2)).astype(T)
        iy = ((((gy + T(1)).astype(T) * T(H)).astype(T) - T(1)).astype(T) / T(2)).astype(T)
        D1 = bilinear_zeros(np.asarray(prob["bias1"], np.float32), ix, iy, T)
        rx, ry = np.rint(ix), np.rint(iy)                                       # half to even
        ok = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)              # False for a NaN
        m = _tap(np.asarray(prob["mask"], np.float32).astype(T), ry, rx, ok)
        valid = (m * pos.astype(T)).astype(T)
        selected = valid > T(0.5)
        ratio = ((z * valid).astype(T) / D1).astype(T)
    return dict(z=z, pos=pos, ix=ix, iy=iy, D1=D1, m=m, valid=valid, selected=selected, ratio=ratio)


def stats(prob, dtype=np.float64, drop_nan=False, pts=None):
    """the fields of ``SageDepthScaleStats`` in ``dtype``"""
    p = points(prob, dtype) if pts is None else pts
    sel = p["ratio"][p["selected"]]
    med, n_used, n_nan = lower_median(sel, drop_nan)
    return dict(ratio=med, n_points=int(p["z"].size), n_pos_depth=int(p["pos"].sum()), n_selected=int(p["selected"].sum()),
                n_nan=n_nan, n_used=n_used)


def _d1_class(img, ix, iy):
    d = bilinear_zeros(img, ix, iy, np.float64)
    return np.where(np.isnan(d), 2, np.where(d == 0, 1, 0))


def ambiguous(prob):
    """[M] bool from the fp64 restatement: points that fp32 may decide either way --
    the nearest tap's coordinate within 1e-4 px of a half-integer while within a pixel of the image (this includes the taps
    at the image border, where one rounding decides in or out); X.z within 1e-4 of eps; and a bilinear coordinate within
    1e-4 px of an integer where the neighbouring cell's taps would change whether D1 is zero, NaN or an ordinary number (a
    zero patch or a NaN texel comes under a tap of weight ~0)"""
    p = points(prob, np.float64)
    cam = prob["cam"]
    w, h = float(cam.w), float(cam.h)
    img = np.asarray(prob["bias1"], np.float32)
    with np.errstate(invalid="ignore"):
        def near_half(u, size):
            frac = np.abs(u - np.floor(u) - 0.5)
            return (frac < 1e-4) & (u > -1.5) & (u < size + 0.5)
        amb = near_half(p["ix"], w) | near_half(p["iy"], h) | (np.abs(p["z"] - float(prob["eps"])) < 1e-4)
        near_int = (np.abs(p["ix"] - np.rint(p["ix"])) < 1e-4) | (np.abs(p["iy"] - np.rint(p["iy"])) < 1e-4)
        fin = np.isfinite(p["ix"]) & np.isfinite(p["iy"])
        cls = [_d1_class(img, p["ix"] + dx, p["iy"] + dy) for dx in (-2e-4, 2e-4) for dy in (-2e-4, 2e-4)]
        differs = np.zeros(len(amb), bool)
        for c in cls[1:]:
            differs |= c != cls[0]
        amb |= near_int & fin & differs
    return amb


def torch_expression(prob, dtype, drop_nan=False):
    """the reference's tensor expressions (mapper.cpp:248-297; mapping_utils.h:855-858 with ``drop_nan``), literally, on torch
    CPU tensors of ``dtype`` -> (ratios [M], selected [M] bool, median) as numpy; the positive-depth mask is taken per point
    ([M], where the reference writes a [M,1] slice)"""
    import torch
    import torch.nn.functional as F
    cam = prob["cam"]
    H, W = int(cam.h), int(cam.w)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dtype)
    rotation, translation = tt(prob["R"]), tt(prob["t"])
    homo0, bias1, mask1 = tt(prob["homo"]), tt(prob["bias1"]), tt(prob["mask"])
    loc = torch.from_numpy(np.asarray(prob["loc1d0"], np.int64))
    valid_dpts_0 = tt(prob["dpt0_map"]).reshape(-1)[loc]
    rotated = torch.matmul(rotation, homo0.permute(1, 0)).permute(1, 0)
    p3d = valid_dpts_0.reshape(-1, 1) * rotated + translation.reshape(1, 3)
    pos = p3d[:, 2] > float(prob["eps"])
    ph = p3d / p3d[:, 2:3]
    x2d = ph[:, 0:1] * float(cam.fx) + float(cam.cx)
    y2d = ph[:, 1:2] * float(cam.fy) + float(cam.cy)
    grid = torch.cat([(x2d + 0.5) * (2.0 / float(cam.w)) - 1.0, (y2d + 0.5) * (2.0 / float(cam.h)) - 1.0], 1).reshape(1, 1, -1, 2)
    dpts1 = F.grid_sample(bias1.reshape(1, 1, H, W), grid, mode="bilinear", padding_mode="zeros", align_corners=False).reshape(-1)
    vmask = F.grid_sample(mask1.reshape(1, 1, H, W), grid, mode="nearest", padding_mode="zeros", align_corners=False).reshape(-1) * pos
    ratios = ((p3d[:, 2] * vmask) / dpts1).reshape(-1)
    nz = torch.nonzero(vmask > 0.5).reshape(-1)
    sel = ratios[nz]
    if drop_nan:
        sel = sel[torch.nonzero(torch.isnan(sel) < 0.5).reshape(-1)]
    med = torch.median(sel)                    # (of an empty tensor: NaN)
    selected = np.zeros(ratios.numel(), bool)
    selected[nz.numpy()] = True
    return ratios.numpy(), selected, med.numpy()[()]
