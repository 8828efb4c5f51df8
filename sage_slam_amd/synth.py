"""Synthetic keyframe windows for the dense-BA hot path (tests + bench data).

The reference ships no TorchScript nets and no data, so
every test and benchmark runs on synthetic keyframes built here, in the layouts
the reference's ``Frame``/``Keyframe`` structs hold (SURVEY.md s8 a10,
``core/mapping/frame.h:17-125``):

* ``feat_pyr  [FS, P]``      feature pyramid, levels concatenated fine->coarse
* ``grad_pyr  [2, FS, P]``   central-difference gradients (x then y)
* ``bias      [H*W]``, ``basis [H*W, CS]``, ``code [CS]``, ``scale``
* ``loc1d     [N]`` int64, ``homo [N, 3]`` sampled source pixels
* shared ``mask [H, W]`` (destination validity), ``level_offsets [L]``, camera pyramid
* ``pose_wk`` = world-from-keyframe ``(R, t)``

The scene is a textured plane seen from cameras on a smooth arc: feature maps are
geometrically consistent across keyframes (``feat_k(pixel) = F(world point)``) and
the true depth lies in the span of the linear depth code, so LM on the window
actually converges (the survey's "realistic gradients matter" note, s7).

This module is host-side *data generation* (numpy); it is not on the hot path.
The pyramid/gradient producer mirrors ``Mapper::GenerateGaussianPyramidWithGrad``
(``core/mapping/mapper.cpp:1384-1426``) and ``ComputeSpatialGrad``
(``core/mapping/mapping_utils.h:236-252``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

F32 = np.float32


# --------------------------------------------------------------------------- cameras
@dataclass
class Camera:
    """``PinholeCamera<float>`` (``common/pinhole_camera.h:44-131``)."""
    fx: float
    fy: float
    cx: float
    cy: float
    w: float
    h: float

    def as_array(self) -> np.ndarray:
        return np.array([self.fx, self.fy, self.cx, self.cy, self.w, self.h], dtype=F32)


def camera_pyramid(cam: Camera, levels: int) -> List[Camera]:
    """``CameraPyramid`` ctor (``common/camera_pyramid.h:18-32``): level i is level i-1
    resized to ``(size_t)(w/2), (size_t)(h/2)`` with fx,u0 / fy,v0 scaled by the ratio
    (``pinhole_camera_impl.h:120-132``), all in fp32."""
    out = [Camera(*[F32(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])]
    for _ in range(1, levels):
        p = out[-1]
        nw = int(F32(p.w) / F32(2))
        nh = int(F32(p.h) / F32(2))
        xr = F32(nw) / F32(p.w)
        yr = F32(nh) / F32(p.h)
        out.append(Camera(F32(p.fx * xr), F32(p.fy * yr), F32(p.cx * xr), F32(p.cy * yr), F32(nw), F32(nh)))
    return out


def level_offsets_of(cams: List[Camera]) -> Tuple[np.ndarray, int]:
    sizes = [int(c.w) * int(c.h) for c in cams]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int32)
    return offs, int(sum(sizes))


# --------------------------------------------------------------------------- producers
def spatial_grad(img: np.ndarray) -> np.ndarray:
    """img [C,H,W] -> [2,C,H,W]; 0.5*(next-prev) with replicate padding, x then y."""
    p = np.pad(img, ((0, 0), (1, 1), (1, 1)), mode="edge")
    gx = F32(0.5) * (p[:, 1:-1, 2:] - p[:, 1:-1, :-2])
    gy = F32(0.5) * (p[:, 2:, 1:-1] - p[:, :-2, 1:-1])
    return np.stack([gx, gy], 0).astype(F32)


_G = (np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=F32) / F32(16.0)).astype(F32)


def _conv_s2(img: np.ndarray) -> np.ndarray:
    """3x3 Gaussian, stride 2, zero pad 1 on [C,H,W] -> [C, H // 2, W // 2] (an odd last row / column is dropped: the size the
    camera pyramid gives the level, ``common/camera_pyramid.h:26-27``)."""
    C, H, W = img.shape
    p = np.pad(img, ((0, 0), (1, 1), (1, 1)))
    h2, w2 = H // 2, W // 2
    out = np.zeros((C, h2, w2), dtype=F32)
    for dy in range(3):
        for dx in range(3):
            out += _G[dy, dx] * p[:, dy:dy + 2 * h2:2, dx:dx + 2 * w2:2]
    return out


def gaussian_pyramid_with_grad(feat: np.ndarray, mask: np.ndarray, levels: int, allow_odd: bool = False):
    """feat [FS,H,W], mask [H,W] -> (pyr [FS,P], grad [2,FS,P]).  Masked stride-2
    Gaussian: level k+1 = conv(level_k * mask_k) / (conv(mask_k) + 1e-8); the mask
    pyramid is nearest-neighbour decimation (source index 2i)."""
    FS, H, W = feat.shape
    # (allow_odd: test inputs with NON-DYADIC camera pyramids, w = 62 -> 31 -> 15 -- levels cropped to the camera pyramid's
    #  floor sizes; the reference's own producer disagrees with its camera pyramid there, the factor kernels do not care)
    assert allow_odd or (H % (1 << (levels - 1)) == 0 and W % (1 << (levels - 1)) == 0), \
        "level sizes must stay even (the reference's conv/camera/mask pyramids only agree then)"
    cur = feat.astype(F32)
    curm = mask.astype(F32)
    pyr, grad = [], []
    for l in range(levels):
        g = spatial_grad(cur)
        pyr.append(cur.reshape(FS, -1))
        grad.append(g.reshape(2, FS, -1))
        if l == levels - 1:
            break
        raw = _conv_s2(cur * curm[None])
        rm = _conv_s2(curm[None])
        cur = (raw / (rm + F32(1.0e-8))).astype(F32)
        curm = curm[::2, ::2][:cur.shape[1], :cur.shape[2]].copy()
    return np.ascontiguousarray(np.concatenate(pyr, 1)), np.ascontiguousarray(np.concatenate(grad, 2))


# --------------------------------------------------------------------------- SE3 helpers (fp64 on host)
def so3_exp(w: np.ndarray) -> np.ndarray:
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


# --------------------------------------------------------------------------- data model
@dataclass
class Keyframe:
    feat_pyr: np.ndarray
    grad_pyr: np.ndarray
    bias: np.ndarray
    basis: np.ndarray
    code: np.ndarray
    scale: float
    loc1d: np.ndarray
    homo: np.ndarray
    R: np.ndarray
    t: np.ndarray
    # ground truth (for convergence tests)
    code_true: np.ndarray = None
    scale_true: float = 1.0
    R_true: np.ndarray = None
    t_true: np.ndarray = None


@dataclass
class Window:
    H: int
    W: int
    L: int
    FS: int
    CS: int
    cams: List[Camera]
    level_offsets: np.ndarray
    P: int
    mask: np.ndarray                      # [H,W] video mask (destination validity)
    keyframes: List[Keyframe]
    links: List[Tuple[int, int]] = field(default_factory=list)   # undirected (older, newer)
    photo_weights: np.ndarray = None      # [L]
    geo_weight: float = 0.1
    geo_loss_param: float = 0.03
    eps: float = 1.0e-4

    def directed_edges(self) -> List[Tuple[int, int]]:
        """Each link contributes both directions (``core/mapping/mapper.cpp:346-374``)."""
        out = []
        for a, b in self.links:
            out.append((a, b))
            out.append((b, a))
        return out


def _texture(rng, FS, n_waves, kmin, kmax):
    ang = rng.uniform(0, 2 * np.pi, (FS, n_waves))
    kk = rng.uniform(kmin, kmax, (FS, n_waves))
    k = np.stack([kk * np.cos(ang), kk * np.sin(ang)], -1)          # [FS,J,2] cycles / world unit
    phase = rng.uniform(0, 2 * np.pi, (FS, n_waves))
    amp = rng.uniform(0.5, 1.0, (FS, n_waves))
    amp /= np.sqrt((amp ** 2).sum(1, keepdims=True))
    return k, phase, amp


def _smooth_fields(rng, n, H, W, sigma, max_cycles=2.0, n_waves=4):
    """n smooth random fields over the image, std ~= sigma."""
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    out = np.zeros((n, H, W))
    for i in range(n):
        f = np.zeros((H, W))
        for _ in range(n_waves):
            kx, ky = rng.uniform(-max_cycles, max_cycles, 2)
            f += rng.uniform(0.5, 1.0) * np.sin(2 * np.pi * (kx * xx + ky * yy) + rng.uniform(0, 2 * np.pi))
        out[i] = f / (f.std() + 1e-12) * sigma
    return out


def make_window(K: int, H: int, W: int, FS: int = 16, CS: int = 32, L: int = 4,
                n_samples: int = 0, back_links: int = 3, seed: int = 0,
                baseline: float = 0.025, pose_noise: float = 1.0, code_noise: float = 0.03,
                border: int = 2, erode: int = 6, loop_radius: float = 0.0, allow_odd: bool = False) -> Window:
    """Build a K-keyframe window (SURVEY.md s8d "synthetic inputs").

    ``n_samples == 0`` -> dense sampling (all pixels of the eroded mask, row-major like
    ``torch.nonzero``); otherwise a seeded shuffle keeps the first ``n_samples``
    (``core/mapping/mapper.cpp:1222-1237``).  ``loop_radius > 0``: the camera walks once around a circle of that
    radius in the x-y plane (keyframe K-1 ends next to keyframe 0: loop closures have overlap) instead of along the
    smooth arc."""
    rng = np.random.default_rng(seed)
    cam0 = Camera(0.9 * W, 0.9 * W, W / 2.0, H / 2.0, W, H)
    cams = camera_pyramid(cam0, L)
    offs, P = level_offsets_of(cams)
    fx, fy, cx, cy = float(cams[0].fx), float(cams[0].fy), float(cams[0].cx), float(cams[0].cy)

    # masks: destination validity = video mask, sampling from the eroded one
    mask = np.zeros((H, W), dtype=F32)
    mask[border:H - border, border:W - border] = 1
    smask = np.zeros((H, W), dtype=bool)
    smask[border + erode:H - border - erode, border + erode:W - border - erode] = True
    valid = np.nonzero(smask.reshape(-1))[0].astype(np.int64)

    # scene: tilted plane n.X = h, texture on in-plane coordinates
    n = np.array([0.08, -0.05, 1.0])
    n /= np.linalg.norm(n)
    h = 1.0
    e1 = np.cross(n, [0, 1, 0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    px = h / fx                                   # world units per pixel at depth ~h
    kvec, phase, amp = _texture(rng, FS, 6, 1.0 / (48 * px), 1.0 / (10 * px))

    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx)], -1)      # [H,W,3]

    kfs: List[Keyframe] = []
    for k in range(K):
        # smooth arc, small rotations that keep the plane in view
        s = k * baseline
        t_true = np.array([s, 0.15 * baseline * np.sin(0.7 * k), 0.05 * baseline * np.cos(0.3 * k)])
        if loop_radius > 0:
            th = 2 * np.pi * k / K
            t_true = np.array([loop_radius * np.sin(th), loop_radius * (1 - np.cos(th)), 0.05 * baseline * np.cos(0.3 * k)])
        R_true = so3_exp(np.array([0.01 * np.sin(0.5 * k), -0.02 * np.sin(0.2 * k), 0.015 * np.sin(0.3 * k)]))
        dirs = rays @ R_true.T
        depth = (h - n @ t_true) / (dirs @ n)                                  # z-depth along the ray
        Xw = dirs * depth[..., None] + t_true
        uv = np.stack([Xw @ e1, Xw @ e2], -1)                                   # [H,W,2]
        arg = 2 * np.pi * np.einsum("hwd,cjd->cjhw", uv, kvec) + phase[:, :, None, None]
        feat = (amp[:, :, None, None] * np.sin(arg)).sum(1).astype(F32)         # [FS,H,W] in [-1,1]
        pyr, grad = gaussian_pyramid_with_grad(feat, mask, L, allow_odd)

        krng = np.random.default_rng(seed * 100003 + k)                         # seed = kf id
        basis = _smooth_fields(krng, CS, H, W, 0.05).reshape(CS, -1).T          # [HW,CS]
        code_true = krng.normal(0, 0.1, CS)
        scale_true = float(np.median(depth))
        bias = depth.reshape(-1) / scale_true - basis @ code_true

        if n_samples and n_samples < valid.size:
            perm = krng.permutation(valid.size)[:n_samples]
            loc = valid[perm]
        else:
            loc = valid
        import os as _os
        if _os.environ.get("SAGE_SYNTH_SHUFFLE") == "1":                        # dev experiment: same samples, shuffled order
            loc = loc[krng.permutation(loc.size)]
        _tile = int(_os.environ.get("SAGE_SYNTH_TILE_ORDER", "0"))              # dev experiment: 2-D tile order of the samples
        if _tile:
            ty, tx = (loc // W) // _tile, (loc % W) // _tile
            loc = loc[np.lexsort((loc % W, loc // W, tx, ty))]
        lx = (loc % W).astype(np.float64)
        ly = (loc // W).astype(np.float64)
        homo = np.stack([(lx - cx) / fx, (ly - cy) / fy, np.ones_like(lx)], -1)

        # perturbed initial estimate
        dw = krng.normal(0, 0.003 * pose_noise, 3)
        dv = krng.normal(0, 0.004 * pose_noise, 3)
        if k == 0:
            dw[:] = 0
            dv[:] = 0
        R0 = so3_exp(dw) @ R_true
        t0 = t_true + dv
        code0 = code_true + krng.normal(0, code_noise, CS)
        scale0 = scale_true * (1 + krng.normal(0, 0.01 * pose_noise))

        kfs.append(Keyframe(
            feat_pyr=pyr, grad_pyr=grad,
            bias=bias.astype(F32), basis=np.ascontiguousarray(basis, dtype=F32),
            code=code0.astype(F32), scale=float(F32(scale0)),
            loc1d=loc.astype(np.int64), homo=homo.astype(F32),
            R=R0.astype(F32), t=t0.astype(F32),
            code_true=code_true.astype(F32), scale_true=scale_true,
            R_true=R_true.astype(F32), t_true=t_true.astype(F32)))

    links = [(j, i) for i in range(K) for j in range(max(0, i - back_links), i)]
    bias2 = float(np.mean([np.mean((kf.scale * kf.bias) ** 2) for kf in kfs]))
    return Window(H=H, W=W, L=L, FS=FS, CS=CS, cams=cams, level_offsets=offs, P=P, mask=mask,
                  keyframes=kfs, links=links,
                  photo_weights=np.array([10, 9, 8, 7, 6, 5][:L], dtype=F32),
                  geo_weight=0.1, geo_loss_param=float(0.03 * bias2), eps=1.0e-4)


def relative_pose(R0, t0, R1, t1):
    """``R10 = R1^T R0``, ``t10 = R1^T (t0 - t1)`` in fp32
    (``core/gtsam/photometric_factor.cpp:280-281``)."""
    R0 = R0.astype(F32); R1 = R1.astype(F32)
    return (R1.T @ R0).astype(F32), (R1.T @ (t0.astype(F32) - t1.astype(F32))).astype(F32)


def depth_and_grad(kf: Keyframe, H: int, W: int):
    """Caller-side precompute of the geometric factor (``geometric_factor.cpp:317-347``):
    ``D1 = s1*(bias1 + basis1*code1)`` and ``gradD1 = s1*centraldiff(bias1 + basis1*code1)``."""
    unscaled = (kf.bias + kf.basis @ kf.code).astype(F32).reshape(1, H, W)
    g = spatial_grad(unscaled)[:, 0]
    return (F32(kf.scale) * unscaled[0]).astype(F32), (F32(kf.scale) * g).astype(F32)


# --------------------------------------------------------------------------- matched keypoints (window keypoint terms)
def _project_true(w: Window, k0: int, k1: int, n: int, seed: int, noise_px: float, outlier_share: float):
    """n keypoints drawn from keyframe k0's samples, projected into k1 with the window's TRUE variables, plus pixel noise;
    a share of the matches is replaced by uniform gross outliers -> (loc0 int32 [n], homo0 [n,3], pixels in k1 [n,2])."""
    a, b = w.keyframes[k0], w.keyframes[k1]
    rng = np.random.default_rng([seed, k0, k1, n])
    pick = rng.choice(a.loc1d.size, size=n, replace=n > a.loc1d.size)
    loc0 = a.loc1d[pick].astype(np.int64)
    homo0 = a.homo[pick].astype(np.float64)
    d = float(a.scale_true) * (a.bias[loc0].astype(np.float64) + a.basis[loc0].astype(np.float64) @ a.code_true.astype(np.float64))
    Xw = (a.R_true.astype(np.float64) @ (d[:, None] * homo0).T).T + a.t_true.astype(np.float64)
    X1 = (b.R_true.astype(np.float64).T @ (Xw - b.t_true.astype(np.float64)).T).T
    cam = w.cams[0]
    px = np.stack([X1[:, 0] / X1[:, 2] * float(cam.fx) + float(cam.cx), X1[:, 1] / X1[:, 2] * float(cam.fy) + float(cam.cy)], 1)
    px = px + rng.normal(0.0, noise_px, px.shape)
    n_out = int(round(outlier_share * n))
    if n_out > 0:
        bad = rng.choice(n, size=n_out, replace=False)
        px[bad] = np.stack([rng.uniform(0, w.W - 1, n_out), rng.uniform(0, w.H - 1, n_out)], 1)
    return loc0.astype(np.int32), homo0.astype(F32), px


def make_reprojection_matches(w: Window, k0: int, k1: int, n: int, seed: int, noise_px: float = 1.0,
                              outlier_share: float = 0.1) -> dict:
    """Matches of a reprojection term on the directed edge k0 -> k1 (what the reference's factor is constructed with,
    ``core/gtsam/reprojection_factor.cpp:41-188``): dict(kind, loc0 [n] int32, homo0 [n,3], matched_2d [n,2] pixels in k1).
    Deterministic per (seed, k0, k1, n)."""
    loc0, homo0, px = _project_true(w, k0, k1, n, seed, noise_px, outlier_share)
    return dict(kind="reprojection", loc0=loc0, homo0=homo0, matched_2d=px.astype(F32))


def make_match_geometry_matches(w: Window, k0: int, k1: int, n: int, seed: int, noise_px: float = 1.0,
                                outlier_share: float = 0.1) -> dict:
    """Matches of a match-geometry term: the match is the rounded in-image pixel of k1 with its ray ->
    dict(kind, loc0 [n] int32, homo0 [n,3], loc1 [n] int32, homo1 [n,3])."""
    loc0, homo0, px = _project_true(w, k0, k1, n, seed, noise_px, outlier_share)
    cam = w.cams[0]
    x = np.clip(np.rint(px[:, 0]), 0, w.W - 1).astype(np.int64)
    y = np.clip(np.rint(px[:, 1]), 0, w.H - 1).astype(np.int64)
    homo1 = np.stack([(x - float(cam.cx)) / float(cam.fx), (y - float(cam.cy)) / float(cam.fy), np.ones(n)], 1)
    return dict(kind="match_geometry", loc0=loc0, homo0=homo0, loc1=(y * w.W + x).astype(np.int32), homo1=homo1.astype(F32))


# --------------------------------------------------------------------------- loop-MG terms (fixed depths, D = 14)
def _unscaled_depths(kf: Keyframe, loc: np.ndarray, code: np.ndarray) -> np.ndarray:
    """``bias[loc] + basis[loc] . code`` in fp32: the depths a loop-closure graph fixes when it is built
    (``matched_unscaled_dpts``, ``core/deepfactors.cpp:388-575``)."""
    loc = np.asarray(loc, np.int64)
    return (kf.bias[loc].astype(F32) + kf.basis[loc].astype(F32) @ np.asarray(code, F32)).astype(F32)


def make_loop_mg_terms_from_matches(w: Window, k0: int, k1: int, n: int, seed: int, noise_px: float = 1.0,
                                    outlier_share: float = 0.1) -> dict:
    """A loop-MG term on the directed edge k0 -> k1 from the matches of ``make_match_geometry_matches``: the two depth
    arrays are formed at the window's INITIAL codes, ``u0 = bias0[loc0] + basis0[loc0] . code0`` and
    ``u1 = bias1[loc1] + basis1[loc1] . code1`` (fp32) -> dict(kind, loc0, loc1, homo0 [n,3], homo1 [n,3], u0 [n], u1 [n]).
    With pixel noise and outliers the residuals are large: data for parity checks, not for a recovery test."""
    m = make_match_geometry_matches(w, k0, k1, n, seed, noise_px, outlier_share)
    a, b = w.keyframes[k0], w.keyframes[k1]
    return dict(kind="loop_mg", loc0=m["loc0"], loc1=m["loc1"], homo0=m["homo0"], homo1=m["homo1"],
                u0=_unscaled_depths(a, m["loc0"], a.code), u1=_unscaled_depths(b, m["loc1"], b.code))


def make_loop_mg_exact(w: Window, k0: int, k1: int, n: int, seed: int) -> dict:
    """A loop-MG term whose residual vanishes at the window's TRUE poses and scales: n points of keyframe k0's samples with
    ``u0`` from the true code; the matched ray and depth are the exact true point in k1, ``homo1 = X1 / X1.z`` and
    ``u1 = X1.z / scale_true(k1)`` (no pixel rounding) -> dict(kind, loc0, homo0, homo1, u0, u1).  Deterministic per
    (seed, k0, k1, n)."""
    a, b = w.keyframes[k0], w.keyframes[k1]
    rng = np.random.default_rng([seed, k0, k1, n, 14])
    pick = rng.choice(a.loc1d.size, size=n, replace=n > a.loc1d.size)
    loc0 = a.loc1d[pick].astype(np.int64)
    homo0 = a.homo[pick].astype(F32)
    u0 = _unscaled_depths(a, loc0, a.code_true)
    d = float(a.scale_true) * u0.astype(np.float64)
    Xw = (a.R_true.astype(np.float64) @ (d[:, None] * homo0.astype(np.float64)).T).T + a.t_true.astype(np.float64)
    X1 = (b.R_true.astype(np.float64).T @ (Xw - b.t_true.astype(np.float64)).T).T
    return dict(kind="loop_mg", loc0=loc0.astype(np.int32), homo0=homo0, homo1=(X1 / X1[:, 2:3]).astype(F32),
                u0=u0, u1=(X1[:, 2] / float(b.scale_true)).astype(F32))


# --------------------------------------------------------------------------- pose-graph terms (the reference's live loop-closure graph)
def _pose12(R, t) -> np.ndarray:
    return np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)])


def _rel12(p0: np.ndarray, p1: np.ndarray) -> np.ndarray:
    """``pose1^-1 * pose0`` of two poses [R row-major | t] in fp64"""
    R0, R1 = p0[:9].reshape(3, 3), p1[:9].reshape(3, 3)
    return np.concatenate([(R1.T @ R0).reshape(-1), R1.T @ (p0[9:] - p1[9:])])


def make_pose_graph(w: Window, links, loops=(), local_targets: str = "start", drift: float = 0.0, seed: int = 0,
                    local_weight: float = 1.0, global_weight: float = 5.0, rot_weight: float = 1.0, scale_weight: float = 3.0,
                    anchor_weight: float = 100.0, scale_prior_weight: float = 50.0):
    """The graph of ``DeepFactors::LoopClosurePoseScaleEstimate`` (``core/deepfactors.cpp:58-386``) on the keyframes of ``w``
    as window graph terms (``capi.Window(graph_terms=...)``); default weights are ``configs/slam_run.flags:63-67``.

    * start: ``w``'s current estimates, or -- ``drift > 0`` -- the TRUE poses and scales under a drift that accumulates along
      the keyframes (per keyframe a world-side twist ~ N(0, drift^2)_6 and a log-scale step ~ N(0, drift^2); keyframe 0 exact);
    * local ``links``: two ``rel_pose_scale`` terms each (the second with the inverse target and the scales swapped) whose
      target is the relative pose and the scales of the start (``local_targets="start"``: on target, as the reference builds
      them, ``deepfactors.cpp:126-183``) or of the truth (``"truth"``);
    * ``loops``: links appended behind the local ones, terms of ``global_weight`` whose target is the TRUE relative pose and
      scales (the tracker's measurement: it disagrees with a drifted chain, ``:236-272``);
    * a ``scale_prior`` of ``anchor_weight`` on keyframe 0 at its start scale (``:119``) and, with loops, two of
      ``scale_prior_weight`` on the first loop's keyframes at their true scales (``:277-282``).

    -> (window with the start variables and no dense link, all links, terms, holds): every code held, keyframe 0's pose held
    (the reference's sigma = 1e-4 pose prior).  Deterministic per ``seed``."""
    import dataclasses
    assert local_targets in ("start", "truth")
    rng = np.random.default_rng([seed, len(w.keyframes), 77])
    truth = [(_pose12(kf.R_true, kf.t_true), float(kf.scale_true)) for kf in w.keyframes]
    start = [(_pose12(kf.R, kf.t), float(kf.scale)) for kf in w.keyframes]
    if drift > 0:
        DR, Dt, ds = np.eye(3), np.zeros(3), 1.0
        start = []
        for k, (p, s) in enumerate(truth):
            if k > 0:
                xi = rng.normal(0.0, drift, 6)
                dR = so3_exp(xi[3:])
                DR, Dt, ds = dR @ DR, dR @ Dt + xi[:3], ds * float(np.exp(rng.normal(0.0, drift)))
            start.append((_pose12(DR @ p[:9].reshape(3, 3), DR @ p[9:] + Dt), s * ds))
    # (what the engine holds is fp32: targets "on the start" are formed from the rounded variables)
    start = [(p.astype(F32).astype(np.float64), float(F32(s))) for p, s in start]
    kfs = [dataclasses.replace(kf, R=p[:9].reshape(3, 3).astype(F32), t=p[9:].astype(F32), scale=s)
           for kf, (p, s) in zip(w.keyframes, start)]
    all_links = [(min(a, b), max(a, b)) for a, b in list(links) + list(loops)]
    terms = []
    for l, (a, b) in enumerate(all_links):
        is_loop = l >= len(links)
        src = truth if (is_loop or local_targets == "truth") else start
        for d, (k0, k1) in enumerate(((a, b), (b, a))):
            terms.append(dict(kind="rel_pose_scale", edge=2 * l + d, target_pose10=_rel12(src[k0][0], src[k1][0]).astype(F32),
                              target_scale0=float(F32(src[k0][1])), target_scale1=float(F32(src[k1][1])),
                              weight=global_weight if is_loop else local_weight, rot_weight=rot_weight, scale_weight=scale_weight))
    terms.append(dict(kind="scale_prior", kf=0, target_scale0=start[0][1], weight=anchor_weight))
    if loops:
        a, b = all_links[len(links)]
        for k in (a, b):
            terms.append(dict(kind="scale_prior", kf=k, target_scale0=float(F32(truth[k][1])), weight=scale_prior_weight))
    holds = {k: 2 for k in range(len(kfs))}       # SAGE_HOLD_CODE
    holds[0] = 1 | 2                              # ... and keyframe 0's pose
    return dataclasses.replace(w, keyframes=kfs, links=[]), all_links, terms, holds


# --------------------------------------------------------------------------- overlap statistics of a tracked pose
OVERLAP_POSES = {              # name -> (rotation vector, translation): near, far, and mostly behind the camera
    "small": ((0.02, -0.03, 0.05), (0.05, -0.02, 0.03)),
    "big": ((0.1, 0.25, 0.4), (0.4, 0.1, -0.2)),
    "behind": ((0.0, 0.9, 0.0), (0.2, 0.0, -0.9)),
}


def make_overlap_problem(H: int, W: int, rot=(0.0, 0.0, 0.0), trans=(0.0, 0.0, 0.0), seed: int = 0) -> dict:
    """Inputs of ``sage_track_overlap`` (``CameraTracker::ComputeAreaInlierRatio``): the valid set of a keyframe under an
    elliptical video mask ``((x - cx) / 0.48 W)^2 + ((y - cy) / 0.47 H)^2 < 1``, in raster order as
    ``mapping_utils.h:254-287`` enumerates it, camera ``fx = fy = 0.9 W`` centred on the image, depths
    ``1 + 0.3 sin(x / 7) + 0.2 U(0, 1)``, and the pose ``(so3_exp(rot), trans)``.
    -> dict(cam, mask [H,W], dpts0 [M], homo [M,3], R [3,3], t [3], eps, M), everything fp32.  Deterministic per ``seed``."""
    cam = Camera(F32(0.9 * W), F32(0.9 * W), F32(0.5 * (W - 1)), F32(0.5 * (H - 1)), F32(W), F32(H))
    ys, xs = np.mgrid[0:H, 0:W]
    mask = ((((xs - float(cam.cx)) / (0.48 * W)) ** 2 + ((ys - float(cam.cy)) / (0.47 * H)) ** 2) < 1.0).astype(F32)
    vy, vx = np.nonzero(mask > 0.5)
    rng = np.random.default_rng([seed, H, W, 411])
    dpts0 = (1.0 + 0.3 * np.sin(vx / 7.0) + 0.2 * rng.random(vx.size)).astype(F32)
    homo = np.stack([(vx.astype(F32) - cam.cx) / cam.fx, (vy.astype(F32) - cam.cy) / cam.fy, np.ones(vx.size, F32)], 1).astype(F32)
    return dict(cam=cam, mask=mask, dpts0=dpts0, homo=homo, R=so3_exp(np.asarray(rot, np.float64)).astype(F32),
                t=np.asarray(trans, F32), eps=F32(1e-4), M=int(vx.size))


# --------------------------------------------------------------------------- the mapper's depth-scale correction
DEPTH_SCALE_VARIANTS = ("plain", "zero_patch", "nan_texel")


def make_depth_scale_problem(H: int, W: int, pose="small", seed: int = 0, true_scale: float = 1.7, variant: str = "plain") -> dict:
    """Inputs of ``sage_depth_scale_ratio`` (``Mapper::CorrectDepthScale``) with a known answer.  Keyframe 0 is the scene of
    ``make_overlap_problem`` (valid set, depths, homo, elliptical mask, camera); ``pose`` is a name of ``OVERLAP_POSES`` or a
    (rotation vector, translation) pair.  Keyframe 1's ``bias1`` is the depth of that scene seen from pose 1, divided by
    ``true_scale``: keyframe 0's points are warped in fp64, their depths splatted into the pixel they land in (the nearest
    one wins a shared pixel), and the pixels no point reached are filled from their filled 3x3 neighbours' mean, ring by
    ring -- a depth map as good as the scene's sampling allows, so the median ratio is ``true_scale`` up to that
    interpolation error.  Without a point in front of the camera (``behind``) ``bias1`` is 1 everywhere.
    ``variant``: "zero_patch" zeroes a 6x6 patch of ``bias1`` at the image centre (ratios of +inf), "nan_texel" plants one
    NaN next to it (NaN ratios among the selected).
    -> the overlap problem's dict + dpt0_map [H,W] (keyframe 0's depth map, 0 outside the valid set), loc1d0 [M] int64,
    bias1 [H,W], true_scale, variant.  Deterministic per ``seed``."""
    assert variant in DEPTH_SCALE_VARIANTS
    rot, trans = OVERLAP_POSES[pose] if isinstance(pose, str) else pose
    prob = make_overlap_problem(H, W, rot, trans, seed)
    cam = prob["cam"]
    vy, vx = np.nonzero(prob["mask"] > 0.5)
    loc1d0 = (vy * W + vx).astype(np.int64)
    dpt0_map = np.zeros((H, W), F32)
    dpt0_map.reshape(-1)[loc1d0] = prob["dpts0"]
    X = prob["dpts0"].astype(np.float64)[:, None] * (prob["homo"].astype(np.float64) @ prob["R"].astype(np.float64).T) \
        + prob["t"].astype(np.float64)
    front = X[:, 2] > 1e-3
    depth = np.full((H, W), np.inf)
    px = np.rint(X[front, 0] / X[front, 2] * float(cam.fx) + float(cam.cx)).astype(np.int64)
    py = np.rint(X[front, 1] / X[front, 2] * float(cam.fy) + float(cam.cy)).astype(np.int64)
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    np.minimum.at(depth, (py[inside], px[inside]), X[front, 2][inside])
    filled = np.isfinite(depth)
    if not filled.any():
        depth[:], filled[:] = 1.0, True
    for _ in range(H + W):                      # every ring fills the holes next to a filled pixel
        if filled.all():
            break
        d, f = np.pad(np.where(filled, depth, 0.0), 1), np.pad(filled, 1).astype(np.float64)
        s = sum(d[1 + a:1 + a + H, 1 + b:1 + b + W] for a in (-1, 0, 1) for b in (-1, 0, 1))
        n = sum(f[1 + a:1 + a + H, 1 + b:1 + b + W] for a in (-1, 0, 1) for b in (-1, 0, 1))
        new = ~filled & (n > 0)
        depth[new] = s[new] / n[new]
        filled |= new
    bias1 = (depth / float(true_scale)).astype(F32)
    cy, cx = H // 2, W // 2
    if variant == "zero_patch":
        bias1[cy - 3:cy + 3, cx - 3:cx + 3] = 0.0
    elif variant == "nan_texel":
        bias1[cy, cx + 5] = np.nan
    return dict(prob, dpt0_map=dpt0_map, loc1d0=loc1d0, bias1=bias1, true_scale=float(true_scale), variant=variant)


# --------------------------------------------------------------------------- the loop detector's bag of words
BOW_KINDS = ("iid", "nodes", "constant", "nan")


def make_vocabulary(k: int, L: int, C: int, seed: int = 0, ragged: bool = False) -> dict:
    """A vocabulary tree in the arrays ``sage_vocabulary_create`` takes (what ``vocabulary.load_opencv_yaml`` returns).

    Nodes are numbered the way DBoW2's hierarchical k-means numbers them -- a node's children get consecutive ids when the
    node is split, before any of them is split itself -- so the numbering is NOT breadth-first below level 2.  A child's
    descriptor is its parent's plus Gaussian noise of sigma 0.3 / 2^level (the root's row is zero), a leaf's weight is drawn
    from [0.5, 3), an inner node's is 0 as in a DBoW2 file.
    ``ragged`` False: every inner node has k children, every leaf is at depth L, word ids ascend with the node id.
    ``ragged`` True: 1..k children per inner node, a node above depth L is a leaf with probability 0.3 (leaves at depths
    1..L), about one leaf weight in five is 0, and the word ids are a random permutation.
    -> dict(parent, descriptors [n, C], weight, word_id, k, L, scoring = 0 (L1), weighting = 0, n_nodes, n_words, C).
    Deterministic per ``seed``."""
    rng = np.random.default_rng(seed)
    parent, level = [-1], [0]
    desc = [np.zeros(C, np.float64)]
    is_leaf = [False]

    def split(node: int):
        lvl = level[node] + 1
        n = int(rng.integers(1, k + 1)) if ragged else k
        kids = list(range(len(parent), len(parent) + n))
        for _ in kids:
            parent.append(node)
            level.append(lvl)
            desc.append(desc[node] + rng.normal(0.0, 0.3 / 2.0 ** (lvl - 1), C))
            is_leaf.append(lvl >= L or (ragged and rng.random() < 0.3))
        for c in kids:
            if not is_leaf[c]:
                split(c)

    split(0)
    n = len(parent)
    leaves = np.nonzero(np.array(is_leaf))[0]
    words = rng.permutation(len(leaves)) if ragged else np.arange(len(leaves))
    word_id = np.full(n, -1, np.int32)
    word_id[leaves] = words
    weight = np.zeros(n, np.float64)
    weight[leaves] = rng.uniform(0.5, 3.0, len(leaves))
    if ragged:
        weight[leaves[rng.random(len(leaves)) < 0.2]] = 0.0
    return dict(parent=np.array(parent, np.int32), descriptors=np.array(desc).astype(F32), weight=weight, word_id=word_id, k=k, L=L,
                scoring=0, weighting=0, n_nodes=n, n_words=int(len(leaves)), C=C)


VOC_TRAINING_KINDS = ("planted", "iid")


def make_voc_training_set(k: int, L: int, C: int, n_docs: int, per_doc: int, seed: int = 0, kind: str = "planted") -> dict:
    """Training descriptors for ``sage_vocabulary_build``: ``n_docs`` documents of ``per_doc`` points each.
    ``kind`` "planted": a hierarchy of well-separated centres -- level l's centres are their parent's plus Gaussian offsets
    of sigma 4^-(l-1), k per node down to level L --, every point a uniformly drawn level-L centre plus noise of sigma
    0.02 * 4^-(L-1): the clusters k-means should find are far apart next to their own spread at every level.
    "iid": Gaussian descriptors of sigma 0.3 (no structure: many close decisions).
    -> dict(desc [C, M] float32 channel-major, doc_begin [n_docs + 1] int64, M, C, n_docs, kind).  Deterministic per ``seed``."""
    assert kind in VOC_TRAINING_KINDS and k >= 2 and L >= 1 and n_docs >= 1 and per_doc >= 1
    rng = np.random.default_rng(seed)
    M = n_docs * per_doc
    if kind == "iid":
        pts = rng.normal(0.0, 0.3, (M, C))
    else:
        centres = np.zeros((1, C))
        for l in range(1, L + 1):
            centres = (centres[:, None, :] + rng.normal(0.0, 4.0 ** -(l - 1), (centres.shape[0], k, C))).reshape(-1, C)
        pts = centres[rng.integers(0, centres.shape[0], M)] + rng.normal(0.0, 0.02 * 4.0 ** -(L - 1), (M, C))
    return dict(desc=np.ascontiguousarray(pts.T, F32), doc_begin=np.arange(n_docs + 1, dtype=np.int64) * per_doc, M=M, C=C,
                n_docs=n_docs, kind=kind)


def make_bow_problem(H: int, W: int, C: int, seed: int = 0, kind: str = "iid", voc: dict = None) -> dict:
    """Inputs of ``sage_bow_transform`` (``LoopDetector::AddKeyframe``): a descriptor map ``desc`` [C, H*W] (``feat_desc``
    reshaped to {C, -1}) and the valid locations ``loc1d`` [M] (int64, ascending) of the eroded mask of ``make_window`` (8
    pixels off every border: M = (H - 16)(W - 16)).
    ``kind``: "iid": Gaussian descriptors of sigma 0.3 (few words of a trained vocabulary); "nodes": the descriptor of a
    random non-root node of ``voc`` plus noise of sigma 0.15 (most words); "constant": one descriptor at every pixel (one
    word); "nan": "iid" with channel 0 NaN at every pixel (every distance is NaN: child 0 at every level).
    -> dict(desc, mask [H, W] bool, loc1d, M, P, H, W, C, kind).  Deterministic per ``seed``."""
    assert kind in BOW_KINDS and H > 16 and W > 16
    rng = np.random.default_rng(seed)
    P = H * W
    if kind == "nodes":
        assert voc is not None and voc["C"] == C
        pick = rng.integers(1, voc["n_nodes"], P)
        desc = voc["descriptors"][pick].T.astype(np.float64) + rng.normal(0.0, 0.15, (C, P))
    elif kind == "constant":
        desc = np.repeat(rng.normal(0.0, 0.3, (C, 1)), P, axis=1)
    else:
        desc = rng.normal(0.0, 0.3, (C, P))
        if kind == "nan":
            desc[0] = np.nan
    mask = np.zeros((H, W), bool)
    mask[8:H - 8, 8:W - 8] = True
    loc1d = np.nonzero(mask.reshape(-1))[0].astype(np.int64)
    return dict(desc=np.ascontiguousarray(desc, F32), mask=mask, loc1d=loc1d, M=int(loc1d.size), P=P, H=H, W=W, C=C, kind=kind)


REG_VARIANTS = ("plain", "all_outliers", "noise_free", "coincident_dst", "coincident_src", "clamp")


def registration_params(noise_bound: float) -> dict:
    """The reference's shipped solver parameters (configs/slam_run.flags:76-85) around a scalar ``noise_bound``"""
    return dict(noise_bound=float(noise_bound), cbar2=1.0, rotation_max_iterations=20, rotation_cost_threshold=1e-4,
                rotation_gnc_factor=1.4, rotation_tim_graph=0, inlier_selection_mode=3, rotation_algorithm=0)


def make_registration_problem(N: int, seed: int = 0, outlier_rate: float = 0.3, noise: float = 0.3, variant: str = "plain") -> dict:
    """Inputs of ``sage_robust_registration`` as ``CameraTracker::FeatureMatchingGeo`` builds them: ``src`` [N, 3] are points
    d * (x, y, 1) of a camera with focal length 200 (depths 0.5 .. 3, |x|, |y| <= 0.5), ``dst`` = s R src + t plus, per axis,
    uniform noise of ``noise`` times the point's bound; ``noise_bounds`` [N] = max(2 * dst_z / 200, 5e-4) in fp32; a share
    ``outlier_rate`` of the dst points is replaced by points drawn like src.  ``variant``: "plain"; "all_outliers" (every dst
    point replaced); "noise_free" (no noise, no outliers: the GNC leaves at iteration 0); "coincident_dst" (every 8th dst
    point repeats its predecessor: pairs with X = 0); "coincident_src" (every 8th src point repeats its predecessor: pairs
    with v1 = 0); "clamp" (depths 0.01 .. 0.04: every bound sits at the 5e-4 clamp).
    -> dict(src, dst, noise_bounds (float32), params (``registration_params``), scale, R, t (the plant), outlier [N] bool).
    Deterministic per (N, seed, outlier_rate, noise, variant)."""
    assert variant in REG_VARIANTS and N >= 2
    rng = np.random.default_rng([seed, N, REG_VARIANTS.index(variant)])
    mult, focal = 2.0, 200.0
    dlo, dhi = (0.01, 0.04) if variant == "clamp" else (0.5, 3.0)

    def cloud(n):
        d = rng.uniform(dlo, dhi, n)
        return np.stack([d * rng.uniform(-0.5, 0.5, n), d * rng.uniform(-0.5, 0.5, n), d], 1)

    src = cloud(N)
    s = float(rng.uniform(0.7, 1.4))
    R = so3_exp(rng.normal(0.0, 0.15, 3))
    t = rng.normal(0.0, 0.05, 3) * (0.02 if variant == "clamp" else 1.0)
    if variant == "coincident_src":
        src[7::8] = src[6::8][:len(src[7::8])]
    dst = s * src @ R.T + t
    if variant == "noise_free":
        outlier_rate, noise = 0.0, 0.0
    if variant == "all_outliers":
        outlier_rate = 1.0
    n_out = int(round(outlier_rate * N))
    outlier = np.zeros(N, bool)
    outlier[rng.permutation(N)[:n_out]] = True
    repl = cloud(N)
    dst[outlier] = repl[outlier]
    nb = np.maximum((np.float32(mult) * dst[:, 2].astype(F32)) / np.float32(focal), np.float32(5e-4)).astype(F32)
    dst = dst + noise * nb[:, None].astype(np.float64) * rng.uniform(-1.0, 1.0, (N, 3))
    if variant == "coincident_dst":
        dst[7::8] = dst[6::8][:len(dst[7::8])]
    src32, dst32 = np.ascontiguousarray(src, F32), np.ascontiguousarray(dst, F32)
    nb = np.maximum((np.float32(mult) * dst32[:, 2]) / np.float32(focal), np.float32(5e-4)).astype(F32)
    noise_bound = float(np.float32(mult) * np.float32(dst32[:, 2].astype(np.float64).mean()) / np.float32(focal))
    return dict(src=src32, dst=dst32, noise_bounds=nb, params=registration_params(noise_bound), scale=s, R=R, t=t,
                outlier=outlier, N=N, variant=variant)


LOOP_CANDIDATE_KINDS = ("planted", "self", "unrelated")


def make_loop_candidates(seed: int, B: int, H: int = 48, W: int = 64, C: int = 16, K: int = 117, kinds=None, n_wrong: int = 8,
                         grid: int = 4) -> dict:
    """Inputs of ``sage_cycle_match_batch`` / ``sage_loop_precheck``: one query keyframe and B loop-closure candidates.
    The query has a descriptor map [C, H, W] (iid normal), a smooth depth map [H*W] and the pixels of a ``grid``-pixel grid (4; 2
    for more keypoints than a small image has on that) 8 pixels inside the border as possible keypoints; the camera has focal length 0.94 W.  Every candidate draws its own K keypoints from
    that grid (all of them, in raster order, when the grid has exactly K; the reference shuffles the query's valid locations
    with the candidate's id as seed).  ``kinds[b]`` (default: "planted", "self", "unrelated", "planted", ... in turn):
      "planted"    the candidate sees the keypoints under its own similarity (s, R, t): each keypoint's descriptor is planted at
                   the pixel its point projects to (rounded), with that point's depth in the candidate's depth map, in an
                   otherwise unrelated map; ``n_wrong`` keypoints are planted at a wrong pixel with a wrong depth
      "self"       the query's own maps
      "unrelated"  an iid map of half the query's spread and iid depths (two iid maps of ONE distribution are mutual nearest
                   neighbours for about a third of the keypoints at C = 16, which is where the detector's ratio test sits;
                   at half the spread about a tenth of the cycles close)
    -> dict(H, W, C, K, cam, desc_q, dmap_q, depth_divisor (1.0), cands): per candidate dict(kind, desc, dpt_map, kp_loc [K]
    int64, kp_dpts0 [K], kp_homo0 [K, 3], loc1 [K] (where each keypoint was planted; "self": kp_loc; "unrelated": None),
    wrong (sorted positions among the K), s, R, t).  Deterministic per argument set."""
    rng = np.random.default_rng([seed, B, H, W, C, K])
    fx = fy = 0.9375 * W
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    gy, gx = np.meshgrid(np.arange(8, H - 7, grid), np.arange(8, W - 7, grid), indexing="ij")
    gx, gy = gx.reshape(-1), gy.reshape(-1)
    assert 2 <= K <= gx.size and 0 <= n_wrong <= K, (K, gx.size)
    kinds = list(kinds) if kinds is not None else [("planted", "self", "unrelated", "planted")[b % 4] for b in range(B)]
    assert len(kinds) == B and all(k in LOOP_CANDIDATE_KINDS for k in kinds)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dmap_q = (1.5 + 0.3 * np.sin(xx * (7.0 / W)) + 0.2 * np.cos(yy * (7.0 / H))).astype(F32).reshape(-1)
    desc_q = rng.normal(0, 1, (C, H, W)).astype(F32)
    free = np.array([y * W + x for y in range(2, H - 2) for x in range(2, W - 2) if (x % 4 == 1 and y % 4 == 1)], np.int64)
    cands = []
    for b in range(B):
        sel = np.arange(K) if gx.size == K else rng.permutation(gx.size)[:K]
        xs, ys = gx[sel], gy[sel]
        kp = (ys * W + xs).astype(np.int64)
        d0 = dmap_q[kp]
        homo0 = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones(K)], 1).astype(F32)
        c = dict(kind=kinds[b], kp_loc=kp, kp_dpts0=d0, kp_homo0=homo0, loc1=None, wrong=np.zeros(0, np.int64), s=1.0, R=np.eye(3),
                 t=np.zeros(3))
        if kinds[b] == "self":
            c.update(desc=desc_q.copy(), dpt_map=dmap_q.copy(), loc1=kp.copy())
        elif kinds[b] == "unrelated":
            c.update(desc=rng.normal(0, 0.5, (C, H, W)).astype(F32), dpt_map=rng.uniform(1.0, 3.0, H * W).astype(F32))
        else:
            s = float(rng.uniform(0.9, 1.25))
            R = so3_exp(np.clip(rng.normal(0.0, 0.01, 3), -0.015, 0.015))   # (with t: less than the 8 pixels to the border)
            t = np.clip(rng.normal(0.0, 0.015, 3), -0.02, 0.02)
            p1 = s * (d0[:, None].astype(np.float64) * homo0) @ R.T + t
            u1 = np.rint(p1[:, 0] / p1[:, 2] * fx + cx).astype(np.int64)
            v1 = np.rint(p1[:, 1] / p1[:, 2] * fy + cy).astype(np.int64)
            assert u1.min() >= 0 and u1.max() < W and v1.min() >= 0 and v1.max() < H
            wrong = np.sort(rng.permutation(K)[:n_wrong])
            keep = np.ones(K, bool)
            keep[wrong] = False
            pool = np.setdiff1d(free, (v1 * W + u1)[keep])
            pick = pool[rng.permutation(pool.size)[:n_wrong]]
            u1[wrong], v1[wrong] = pick % W, pick // W
            loc1 = v1 * W + u1
            assert np.unique(loc1).size == K
            desc = rng.normal(0, 1, (C, H, W)).astype(F32)
            desc[:, v1, u1] = desc_q[:, ys, xs]
            dmap = np.full(H * W, 2.0, F32)
            dmap[loc1] = p1[:, 2].astype(F32)
            dmap[loc1[wrong]] = rng.uniform(1.0, 3.0, n_wrong).astype(F32)
            c.update(desc=desc, dpt_map=dmap, loc1=loc1, wrong=wrong, s=s, R=R, t=t)
        cands.append(c)
    return dict(H=H, W=W, C=C, K=K, cam=Camera(fx, fy, cx, cy, float(W), float(H)), desc_q=desc_q, dmap_q=dmap_q, depth_divisor=1.0,
                cands=cands)


def make_tsdf_scene(seed: int, dims=(24, 20, 28), hw=(24, 32), n: int = 5, voxel_size: float = 0.04, trunc_voxels: float = 3.0,
                    sigma=(0.02, 0.12), depth_holes: float = 0.10, std_holes: float = 0.05, spread=(0.55, 1.15)) -> dict:
    """Inputs of ``sage_tsdf_integrate`` / ``_batch``: a volume of ``dims`` voxels around a sphere (a smooth surface with an
    analytic ray intersection) and ``n`` views of it.  Nothing is axis-aligned: the origin and the voxel size are no round
    numbers, every camera looks at the volume's centre from a random direction with a random roll and a random tilt of up to
    ~0.2 rad, and the intrinsics are non-integer, so projected coordinates do not land on .5.  The cameras stand ``spread``
    times the volume's half diagonal from the centre: some inside the volume (voxels behind the camera), all with a field of
    view the volume overflows on every side.  A view's depth is the z of the nearest intersection (0 where the ray misses,
    and in ``depth_holes`` of the pixels), its std a smooth field in ``sigma`` (0 in ``std_holes`` of the pixels), its color
    a packed b 65536 + g 256 + r image.
    -> dict(dims, origin [3] f32, voxel_size f32, trunc_margin f32, cam, views): per view dict(depth, std, color [H, W] f32,
    pose12 [12] f32 world-from-camera).  Deterministic per argument set."""
    H, W = hw
    rng = np.random.default_rng([seed, *dims, H, W, n])
    vs = F32(voxel_size * (1.0 + 0.013 * rng.uniform(-1, 1)))
    origin = (np.array([-0.37, 0.21, 1.13]) + 0.1 * rng.uniform(-1, 1, 3)).astype(F32)
    ext = np.array(dims, np.float64) * float(vs)
    centre = origin.astype(np.float64) + 0.5 * ext
    radius = 0.3 * float(ext.min())
    half_diag = 0.5 * float(np.linalg.norm(ext))
    cam = Camera(F32(0.9 * W + rng.uniform(-0.4, 0.4)), F32(0.9 * W + rng.uniform(-0.4, 0.4)), F32((W - 1) / 2 + rng.uniform(-0.3, 0.3)),
                 F32((H - 1) / 2 + rng.uniform(-0.3, 0.3)), F32(W), F32(H))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rays = np.stack([(xx - float(cam.cx)) / float(cam.fx), (yy - float(cam.cy)) / float(cam.fy), np.ones((H, W))], -1)
    views = []
    for i in range(n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        pos = centre + d * half_diag * rng.uniform(*spread)
        z = -d                                                      # looks at the centre ...
        up = rng.normal(size=3)
        x = np.cross(up, z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z], 1) @ so3_exp(rng.uniform(-0.2, 0.2, 3))   # ... rolled and tilted
        o = R.T @ (pos - centre)                                    # the camera's centre from the sphere's, camera axes
        b = rays @ o
        a = np.sum(rays * rays, -1)
        disc = b * b - a * (o @ o - radius * radius)
        lam = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
        depth = np.where((disc > 0) & (lam > 0), lam, 0.0)          # (the rays have z = 1: lambda is the depth)
        depth[rng.uniform(size=(H, W)) < depth_holes] = 0.0
        fy_, fx_ = rng.uniform(0.5, 2.0, 2)
        std = sigma[0] + (sigma[1] - sigma[0]) * (0.5 + 0.5 * np.sin(fx_ * xx * (6.0 / W) + rng.uniform(0, 6)) * np.cos(fy_ * yy * (6.0 / H)))
        std[rng.uniform(size=(H, W)) < std_holes] = 0.0
        rgb = rng.integers(0, 256, (3, H, W)).astype(np.float64)
        views.append(dict(depth=depth.astype(F32), std=std.astype(F32), color=(rgb[2] * 65536 + rgb[1] * 256 + rgb[0]).astype(F32),
                          pose12=np.concatenate([R.reshape(-1), pos]).astype(F32)))
    return dict(dims=tuple(int(v) for v in dims), origin=origin, voxel_size=vs, trunc_margin=F32(float(vs) * trunc_voxels), cam=cam,
                views=views)
