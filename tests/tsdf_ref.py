"""A numpy restatement of TSDF fusion as include/sage_ba.h ("TSDF fusion") specifies it, parametrised by dtype.

With ``dtype=np.float32`` every listed operation is performed once, in the listed order, on fp32 arrays (numpy rounds each
elementwise fp32 operation once, divisions included: there is no fused multiply-add to be had); with ``np.float64`` the same
expressions run in double on the same fp32 inputs.  ``roundf`` is ``trunc(x + copysign(0.5, x))`` on the value widened to
double (exact for an fp32 x: x + 0.5 has at most 25 significant bits).

``integrate`` returns the volumes and, per view, each voxel's decision record: passed, u, v, clipped (dist cut to 1), and
the raw pixel coordinates.  ``ambiguous`` is the set of voxels whose fp32 and fp64 records differ for any view: on those
the two forms compute different things, not the same thing to different precision, so a test's cases must have none."""
import numpy as np


def roundf(x):
    x64 = np.asarray(x, np.float64)
    return np.trunc(x64 + np.copysign(0.5, x64))


def voxel_points(scene, dtype):
    dx, dy, dz = scene["dims"]
    o = np.asarray(scene["origin"], np.float32).astype(dtype)
    vs = dtype(np.float32(scene["voxel_size"]))
    ax = [o[a] + np.arange(d, dtype=np.float32).astype(dtype) * vs for a, d in enumerate((dx, dy, dz))]
    return np.meshgrid(*ax, indexing="ij")


def integrate_view(scene, view, vol, dtype, P=None):
    """one view into vol = dict(tsdf, weight, color) (arrays of ``dtype``, updated in place) -> the decision record"""
    f = dtype
    px, py, pz = P if P is not None else voxel_points(scene, dtype)
    pose = np.asarray(view["pose12"], np.float32).astype(f)
    R, t = pose[:9].reshape(3, 3), pose[9:]
    cam = view.get("cam", scene["cam"])
    fx, fy, cx, cy = [f(np.float32(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy)]
    w, h = int(cam.w), int(cam.h)
    qx, qy, qz = px - t[0], py - t[1], pz - t[2]
    c = [(R[0, k] * qx + R[1, k] * qy) + R[2, k] * qz for k in range(3)]
    min_depth = f(np.float32(view.get("min_depth", 1.0e-4)))
    ok = ~(c[2] < min_depth)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = fx * (c[0] / c[2]) + cx
        y = fy * (c[1] / c[2]) + cy
    ru, rv = roundf(x), roundf(y)
    with np.errstate(invalid="ignore"):
        ok &= (ru >= 0) & (ru < w) & (rv >= 0) & (rv < h)
    u = np.where(ok, ru, 0).astype(np.int64)
    v = np.where(ok, rv, 0).astype(np.int64)
    at = v * w + u
    depth = np.asarray(view["depth"], np.float32).reshape(-1).astype(f)
    d = depth[at]
    if view.get("mask") is not None:
        d = np.where(np.asarray(view["mask"], np.float32).reshape(-1)[at] <= 0.5, f(0), d)
    s = np.asarray(view["std"], np.float32).reshape(-1).astype(f)[at] if view.get("std") is not None else np.ones_like(d)
    s = np.maximum(s, f(np.float32(view.get("std_floor", 0.0))))
    ok &= ~((d <= 0) | (s <= 0))
    diff = d - c[2]
    ok &= ~(diff < -f(np.float32(scene["trunc_margin"])))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = diff / s
    dist = np.minimum(f(1), ratio)
    ow = f(np.float32(view.get("obs_weight", 1.0)))
    w_old = vol["weight"]
    w_new = w_old + ow
    with np.errstate(invalid="ignore"):
        tsdf = (vol["tsdf"] * w_old + dist * ow) / w_new
    if view.get("color") is not None and vol.get("color") is not None:
        nc = np.asarray(view["color"], np.float32).reshape(-1).astype(f)[at]

        def unpack(col):
            b = np.floor(col / f(65536))
            g = np.floor((col - b * f(65536)) / f(256))
            return b, g, col - b * f(65536) - g * f(256)

        new, old = unpack(nc), unpack(vol["color"])
        ch = [np.minimum(roundf((o_ * w_old + n_ * ow) / w_new).astype(f), f(255)) for o_, n_ in zip(old, new)]
        vol["color"] = np.where(ok, ch[0] * f(65536) + ch[1] * f(256) + ch[2], vol["color"])
    vol["tsdf"] = np.where(ok, tsdf, vol["tsdf"])
    vol["weight"] = np.where(ok, w_new, w_old)
    return dict(passed=ok, u=np.where(ok, u, -1), v=np.where(ok, v, -1), clipped=ok & (ratio > 1), x=x, y=y, cz=c[2], diff=diff)


def integrate(scene, views=None, dtype=np.float32, color=False, start=None):
    """all views in order -> (dict(tsdf, weight[, color]), [record per view])"""
    views = scene["views"] if views is None else views
    dims = scene["dims"]
    vol = dict(tsdf=np.zeros(dims, dtype), weight=np.zeros(dims, dtype))
    if color:
        vol["color"] = np.zeros(dims, dtype)
    if start is not None:
        vol = {k: np.asarray(v).astype(dtype) for k, v in start.items()}
    P = voxel_points(scene, dtype)
    recs = [integrate_view(scene, v, vol, dtype, P) for v in views]
    return vol, recs


def ambiguous(scene, views=None, recs32=None, recs64=None):
    """[dims] bool: the voxels whose fp32 and fp64 decision records differ for any view"""
    if recs32 is None:
        recs32 = integrate(scene, views, np.float32)[1]
    if recs64 is None:
        recs64 = integrate(scene, views, np.float64)[1]
    amb = np.zeros(scene["dims"], bool)
    for a, b in zip(recs32, recs64):
        for key in ("passed", "u", "v", "clipped"):
            amb |= a[key] != b[key]
    return amb


def distance(a, b64):
    """max |a - b| / max(1, |b|)"""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b64, np.float64)
    return float(np.max(np.abs(a64 - b64) / np.maximum(1.0, np.abs(b64)))) if a64.size else 0.0


def zero_crossing(profile, coords):
    """the first sign change of ``profile`` from positive to non-positive along ``coords``, linearly interpolated (None: none)"""
    for i in range(len(profile) - 1):
        a, b = float(profile[i]), float(profile[i + 1])
        if a > 0 >= b:
            return float(coords[i]) + (float(coords[i + 1]) - float(coords[i])) * a / (a - b)
    return None


# ---- the committed cases of tests/test_tsdf_ref.py (which checks them) and tests/test_gpu_tsdf.py ----
# name -> (seed, dims, (H, W), views, obs_weight).  The seeds are chosen so that no voxel is ambiguous; test_tsdf_ref.py
# re-checks that on every run and lists what every case must contain.
CASES = {
    "24x20x28": (0, (24, 20, 28), (24, 32), 5, 1.0),
    "33x17x70": (7, (33, 17, 70), (24, 32), 5, 2.5),
    "64x48x80": (2, (64, 48, 80), (24, 32), 7, 1.0),
}
_CACHE = {}


def case(name, n=None):
    """-> dict(scene, views, vol32, rec32, vol64, rec64) of a committed case, computed once per process and left unchanged;
    ``n``: the scene generated with that many views instead (the batch tests; no reference is computed for those)"""
    from sage_slam_amd import synth
    seed, dims, hw, nv, ow = CASES[name]
    key = (name, n)
    if key not in _CACHE:
        scene = synth.make_tsdf_scene(seed, dims, hw, nv if n is None else n)
        for v in scene["views"]:
            v["obs_weight"] = ow
        out = dict(scene=scene, views=scene["views"])
        if n is None:
            out["vol32"], out["rec32"] = integrate(scene, dtype=np.float32, color=True)
            out["vol64"], out["rec64"] = integrate(scene, dtype=np.float64, color=True)
        _CACHE[key] = out
    return _CACHE[key]
