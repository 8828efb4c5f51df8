"""Shared helpers: run the same edge through the CPU oracle (checker) and the HIP engine (product)."""
import numpy as np

from sage_slam_amd import synth


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def oracle_photo(orc, w, k0, k1, jac=True, prec="f32"):
    a, b = w.keyframes[k0], w.keyframes[k1]
    R10, t10 = synth.relative_pose(a.R, a.t, b.R, b.t)
    if jac:
        return orc.photo_jac_error(R10, t10, a.R, a.t, b.R, b.t, a.bias, a.basis, a.code, w.mask, a.loc1d, a.homo,
                                   a.feat_pyr, b.feat_pyr, b.grad_pyr, w.level_offsets, a.scale, w.cams, w.eps,
                                   w.photo_weights, prec=prec)
    e, n = orc.photo_error(R10, t10, a.bias, a.basis, a.code, w.mask, a.loc1d, a.homo, a.feat_pyr, b.feat_pyr,
                           w.level_offsets, a.scale, w.cams, w.eps, w.photo_weights, prec=prec)
    return dict(error=e, num_inliers=n)


def oracle_geo(orc, w, k0, k1, jac=True, prec="f32"):
    a, b = w.keyframes[k0], w.keyframes[k1]
    R10, t10 = synth.relative_pose(a.R, a.t, b.R, b.t)
    D1, g1 = synth.depth_and_grad(b, w.H, w.W)
    if jac:
        return orc.geo_jac_error(R10, t10, a.R, a.t, b.R, b.t, a.bias, a.basis, a.code, D1, g1,
                                 b.basis.reshape(w.H, w.W, w.CS), w.mask, a.loc1d, a.homo, a.scale, b.scale,
                                 w.cams[0], w.eps, w.geo_loss_param, w.geo_weight, prec=prec)
    e, n = orc.geo_error(R10, t10, a.bias, a.basis, a.code, D1, w.mask, a.loc1d, a.homo, a.scale, w.cams[0],
                         w.eps, w.geo_loss_param, w.geo_weight, prec=prec)
    return dict(error=e, num_inliers=n)


def presample_source(orc_or_none, w, kf):
    """[L,N,FS] source features at the sampled pixels (tracker pre-sampling, camera_tracker.cpp:1092-1123);
    numpy bilinear with zero padding == grid_sample(align_corners=False)."""
    L, FS = w.L, w.FS
    N = kf.homo.shape[0]
    out = np.zeros((L, N, FS), np.float32)
    lx = (kf.loc1d % w.W).astype(np.float32); ly = (kf.loc1d // w.W).astype(np.float32)
    for l, cam in enumerate(w.cams):
        Wl, Hl = int(cam.w), int(cam.h)
        u = (lx + np.float32(0.5)) * np.float32(Wl / w.W) - np.float32(0.5)
        v = (ly + np.float32(0.5)) * np.float32(Hl / w.H) - np.float32(0.5)
        xf = np.floor(u).astype(int); yf = np.floor(v).astype(int)
        img = kf.feat_pyr[:, w.level_offsets[l]:w.level_offsets[l] + Wl * Hl].reshape(FS, Hl, Wl)
        acc = np.zeros((FS, N), np.float32)
        for dx, dy in ((0, 0), (1, 1), (0, 1), (1, 0)):
            x = xf + dx; y = yf + dy
            wx = (1 - np.abs(u - x)).astype(np.float32); wy = (1 - np.abs(v - y)).astype(np.float32)
            ok = (x >= 0) & (x < Wl) & (y >= 0) & (y < Hl)
            xs = np.clip(x, 0, Wl - 1); ys = np.clip(y, 0, Hl - 1)
            acc += np.where(ok, wx * wy, 0).astype(np.float32) * img[:, ys, xs]
        out[l] = acc.T
    return out


def damped_delta(H, g, damp):
    """(H + damp*diag(H)) d = g in fp64 (reference LM damping, camera_tracker.cpp:1182)."""
    Hd = H + damp * np.diag(np.diag(H))
    return np.linalg.solve(Hd, g)


def pose_local(origin, other):
    """[t1 - R1 R0^T t0, log(R1 R0^T)] of two poses [R row-major | t] (gtsam_traits.h:78-89), in fp64."""
    origin = np.asarray(origin, np.float64); other = np.asarray(other, np.float64)
    Rr = other[:9].reshape(3, 3) @ origin[:9].reshape(3, 3).T
    th = np.arccos(np.clip(0.5 * (np.trace(Rr) - 1.0), -1.0, 1.0))
    k = 0.5 if th < 1e-8 else th / (2.0 * np.sin(th))
    return np.concatenate([other[9:] - Rr @ origin[9:], k * np.array([Rr[2, 1] - Rr[1, 2], Rr[0, 2] - Rr[2, 0], Rr[1, 0] - Rr[0, 1]])])


def _se3_exp(d6, prec):
    """exp of the twist [v, omega] by the oracle's statement of the reference formula (mapping_utils.h:316-346) -> (dR, dt)"""
    from oracle import oracle as orc
    return orc.se3_exp(d6[3:], d6[:3], prec=prec)


def retract_ref(pose12, d6):
    """The window's pose retraction in fp64: the left update exp([v, omega]) * pose (gtsam_traits.h:45-70,
    camera_tracker.cpp:491-512) of a pose [R row-major | t].  The twist is the fp32-rounded `d6`, as the retract kernel
    casts the fp64 solution before it takes the exponential; everything after that rounding is double."""
    pose = np.asarray(pose12, np.float64).reshape(12)
    dR, dt = _se3_exp(np.asarray(d6, np.float32).astype(np.float64), "f64")
    return np.concatenate([(dR @ pose[:9].reshape(3, 3)).reshape(9), dR @ pose[9:] + dt])


def retract_ref_f32(pose12, d6):
    """fp32 twin of retract_ref, the "fp32 oracle" of the retraction: the oracle's fp32 exponential and a composition in
    numpy float32 with the products summed left to right, as damped_system.h pose_retract writes them."""
    pose = np.asarray(pose12, np.float32).reshape(12)
    dR, dt = _se3_exp(np.asarray(d6, np.float32), "f32")
    R, t = pose[:9].reshape(3, 3), pose[9:]
    Ro = (dR[:, 0:1] * R[0:1, :] + dR[:, 1:2] * R[1:2, :]) + dR[:, 2:3] * R[2:3, :]
    to = ((dR[:, 0] * t[0] + dR[:, 1] * t[1]) + dR[:, 2] * t[2]) + dt
    out = np.concatenate([Ro.reshape(9), to])
    assert out.dtype == np.float32
    return out


def prior_vectors(w, CS, code_w=1e-3, codes=None, pose0=None, scale0=None, pose_w=1e4, scale_w=1e4):
    """Diagonal and gradient additions of the engine's default priors (SageWindowConfig): code prior `code_w` towards zero on
    every keyframe, scale and pose prior 1e4 (`scale_w`, `pose_w`) on keyframe 0 (code_factor.cpp:55-56,99-104;
    scale_factor.cpp:122-124; df_work.cpp:24-34).  The initial values are the window's; `codes` [K, CS], `pose0`
    [R row-major | t] and `scale0` are the current ones where they have moved (after an accepted step): the scale and pose
    priors then have a gradient.  The engine holds its weights as floats: a bar below 1e-7 wants `code_w` as float32(1e-3)."""
    K, B = len(w.keyframes), 7 + CS
    dadd = np.zeros(K * B); gadd = np.zeros(K * B)
    for k, kf in enumerate(w.keyframes):
        idx = np.arange(k * B + 6, k * B + 6 + CS)
        dadd[idx] += code_w
        gadd[idx] += code_w * (0 - (kf.code if codes is None else codes[k]).astype(np.float64))
    kf0 = w.keyframes[0]
    s_init = float(kf0.scale)
    s = s_init if scale0 is None else float(scale0)
    dadd[6 + CS] += scale_w / (s * s)
    dadd[:6] += pose_w
    if scale0 is not None:
        gadd[6 + CS] += scale_w / s * (np.log(s_init) - np.log(s))
    if pose0 is not None:
        init = np.concatenate([np.asarray(kf0.R, np.float32).ravel(), np.asarray(kf0.t, np.float32).ravel()])
        gadd[:6] += pose_w * pose_local(pose0, init)
    return dadd, gadd
