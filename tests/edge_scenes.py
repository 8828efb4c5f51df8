"""Host side of the edge-shape suites of the tracker kernels (tests/test_gpu_tracker_shapes.py) and the keyframe ingest
producers (tests/test_gpu_producer_shapes.py): the case tables, the scene builders and the oracle calls both suites share.
No GPU, no engine library.  tests/test_edge_scenes.py checks on the CPU, against the fp32 oracle alone, that every case has
the property its GPU test relies on (mixed validity, a live last sample that carries weight, masks with dead and half-dead
texels): a passing GPU test then means something.

Tracker scenes: ``synth.make_window(K=2, ..., pose_noise=2.0)`` (the estimate is off the truth: residuals and gradients
of ordinary size), about 20 % random holes in the destination mask, every 7th source depth negative (behind the camera).
The stride starts at index 0 unless that would kill the LAST sample (N = 1, 8, 15, ..., 64, ...): then it starts at 1, the
last sample is what the ragged-tile cases are about."""
import types

import numpy as np

from sage_slam_amd import synth
from tests.helpers import presample_source, rel

TOL_H = 2e-5            # the project's bar for AtA / Atb (tests/test_gpu_parity.py)
TOL_E = 1e-5            # ... and for the error
CHUNK = 1024            # pixels valid_locations_kernel / order_locations_kernel walk per step


# --------------------------------------------------------------------------------------------------------------------
# tracker cases
# --------------------------------------------------------------------------------------------------------------------
def _tc(H, W, FS, L, N, seed=100, **kw):
    return dict(H=H, W=W, FS=FS, L=L, N=N, seed=seed, **kw)


NON_DYADIC = dict(allow_odd=True, border=2, erode=3)      # 62 -> 31 -> 15, 50 -> 25 -> 12 (tests/test_gpu_parity.py)

# The seed of a case is the first from 100 on at which the scene has the three properties tests/test_edge_scenes.py
# demands of it (0 < inliers < N, the last sample an inlier that carries 100 bars of AtA); most take 100 itself.
TRACKER_CASES = (
    [_tc(32, 40, 32, 2, n, s) for n, s in ((1, 100), (2, 100), (63, 101), (64, 100), (65, 100), (255, 100), (256, 104),
                                           (257, 100))]                      # FS = 32: every wave / tile boundary
    + [_tc(64, 80, 16, 4, n, s) for n, s in ((65, 100), (257, 101), (513, 100), (700, 112))]    # FS = 16: ragged tiles
    + [_tc(64, 80, 32, 4, 700, 284),
       _tc(32, 40, 16, 1, 50),                                               # one level
       _tc(50, 62, 32, 3, 0, 101, **NON_DYADIC)])                            # non-dyadic, dense: N = 40 * 52 = 8 tiles + 32
ZERO_INLIER_CASE = TRACKER_CASES[7]                                          # 32x40, FS = 32, N = 257


def tracker_case_id(c):
    return f"{c['H']}x{c['W']}_FS{c['FS']}_L{c['L']}_N{c['N'] or 'dense'}"


def tail_samples(c):
    """How many samples from the end the "AtA moves by 100 bars without them" property is about: the last sample, except
    on the dense case.  No single one of its 1400 inliers carries 100 bars = 2e-3 of AtA (the heaviest: 1.4e-3), so there
    it is the partial last tile (N = 2080 = 8 x 256 + 32) -- and the last sample alone still has to carry two bars: the
    kernel is within one bar of the fp64 oracle with the sample, so it cannot be without it."""
    return 1 if c["N"] else 32


def negative_depth_indices(N):
    """every 7th sample, never the last one"""
    return np.arange(N)[(0 if (N - 1) % 7 else 1)::7]


def tracker_scene(H, W, FS, L, N, seed=100, far=False, **window_kw):
    """-> namespace with everything ``orc.tracker_photo_jac_error`` / ``tracker_photo_error`` take (see oracle_jac below).
    ``far``: the translation moved 50 behind the camera along z: no sample has a positive depth, zero inliers."""
    w = synth.make_window(K=2, H=H, W=W, FS=FS, CS=32, L=L, n_samples=N, seed=seed, pose_noise=2.0, **window_kw)
    rng = np.random.default_rng(seed + 7)
    mask = (w.mask * (rng.uniform(size=w.mask.shape) < 0.8)).astype(np.float32)
    a, b = w.keyframes[0], w.keyframes[1]
    R, t = synth.relative_pose(a.R, a.t, b.R, b.t)
    if far:
        t = (t - np.array([0, 0, 50], np.float32)).astype(np.float32)
    dpts0 = (np.float32(a.scale) * (a.bias + a.basis @ a.code))[a.loc1d].astype(np.float32)
    n = a.homo.shape[0]
    dpts0[negative_depth_indices(n)] = np.float32(-0.4)
    return types.SimpleNamespace(w=w, H=H, W=W, FS=FS, L=L, N=n, R=R, t=t, mask=mask, dpts0=dpts0, homo=a.homo,
                                 feat0s=presample_source(None, w, a), feat1=b.feat_pyr, grad1=b.grad_pyr,
                                 level_offsets=w.level_offsets, cams=w.cams, eps=w.eps, weights=w.photo_weights,
                                 scale0=float(a.scale))


def oracle_jac(orc, s, dof, prec="f32", n=None):
    """the oracle's tracker linearize on the first ``n`` samples of the scene (default: all)"""
    n = s.N if n is None else n
    return orc.tracker_photo_jac_error(dof, s.R, s.t, s.mask, s.dpts0[:n], s.homo[:n], s.feat0s[:, :n], s.feat1, s.grad1,
                                       s.level_offsets, s.cams, s.eps, s.weights, scale0=s.scale0, prec=prec)


def oracle_err(orc, s, prec="f32"):
    return orc.tracker_photo_error(s.R, s.t, s.mask, s.dpts0, s.homo, s.feat0s, s.feat1, s.level_offsets, s.cams, s.eps,
                                   s.weights, prec=prec)


def tracker_bars(orc, s, dof):
    """-> (the fp64 oracle's linearize, its error-only (error, inliers), the fp32 oracle's own distances from them, bars):
    per quantity the bar is max(the project's bar, 4 x the fp32 oracle's own distance from fp64 on this case).  The kernel
    sums in another order with contracted multiply-adds: it gets the project's bar or four times the reference's own
    rounding, whichever is larger."""
    o32, o64 = oracle_jac(orc, s, dof), oracle_jac(orc, s, dof, "f64")
    e32, _ = oracle_err(orc, s)
    e64, n64 = oracle_err(orc, s, "f64")
    own = dict(AtA=rel(o32["AtA"], o64["AtA"]), Atb=rel(o32["Atb"], o64["Atb"]),
               error=abs(o32["error"] - o64["error"]) / abs(o64["error"]), error_only=abs(e32 - e64) / abs(e64))
    bars = dict(AtA=max(TOL_H, 4 * own["AtA"]), Atb=max(TOL_H, 4 * own["Atb"]), error=max(TOL_E, 4 * own["error"]),
                error_only=max(TOL_E, 4 * own["error_only"]))
    return o64, (e64, n64), own, bars


# --------------------------------------------------------------------------------------------------------------------
# the LM run at a second shape
# --------------------------------------------------------------------------------------------------------------------
LM_SCENE = dict(H=32, W=40, FS=32, L=2, n_samples=257, NK=65, seed=38)
# eight times the offset of tests/test_gpu_tracker.py: three steps before the run converges.  Seed 38 is the first of
# 31 .. 42 at which, from this start, no decision of either composition comes within the margin below of a tie
LM_START = dict(rot=(0.032, -0.024, 0.016), trans=(0.032, -0.024, 0.016))
LM_COMPOSITIONS = [(6, True, True), (7, True, True)]        # dof 6 photo + reprojection, dof 7 photo + match geometry
LM_DECISION_MARGIN = 1e-2      # 50 x the 2e-4 the traces are compared with: fp32 noise cannot flip a decision
LM_MIN_ITERS = 3


def recording_callbacks(lin, err):
    """(lin, err) of ``HostScene.oracle_callbacks`` wrapped so that every accept / reject decision of sage_track_lm
    (``candidate_error < error``, inner damping retries included: the trace shows only the last of an iteration) is
    recorded -> (lin, err, decisions), decisions = [(iteration, error, candidate_error)]; the iteration of a decision is
    the number of steps accepted before it."""
    state = dict(cur=None, it=0)
    decisions = []

    def lin2(p, s):
        A, g, e = lin(p, s)
        if state["cur"] is None:
            state["cur"] = e                      # the error is taken from the linearize on the first pass only
        return A, g, e

    def err2(p, s):
        e = err(p, s)
        decisions.append((state["it"], state["cur"], e))
        if e < state["cur"]:
            state["cur"] = e
            state["it"] += 1
        return e

    return lin2, err2, decisions


def decided_iterations(decisions, n_iters):
    """number of leading iterations all of whose decisions have |candidate_error - error| >= 1e-2 error"""
    for it, cur, cand in decisions:
        if abs(cand - cur) < LM_DECISION_MARGIN * cur:
            return it
    return n_iters


# --------------------------------------------------------------------------------------------------------------------
# producer cases
# --------------------------------------------------------------------------------------------------------------------
DEPTH_SHAPES = [(50, 62), (3, 5), (64, 80)]        # 3100 pixels: no multiple of the 32 / 64 a workgroup covers; W < 64
PYRAMID_CASES = [dict(H=40, W=56, L=4, FS=16),     # last level 5 x 7
                 dict(H=32, W=40, L=3, FS=32),
                 dict(H=64, W=80, L=1, FS=16),
                 dict(H=64, W=80, L=2, FS=16),
                 dict(H=50, W=62, L=2, FS=16)]     # last level 25 x 31
MASK_KINDS = ("ones", "synthetic", "holey", "zeros")
LOCATION_SHAPES = [(24, 32), (32, 32), (25, 41), (50, 62)]     # below one chunk, one chunk, one chunk + 1, 3 chunks + 28
LOCATION_MASKS = ("zeros", "ones", "random", "last_pixel", "last_chunk", "threshold")


def depth_inputs(H, W, CS, seed=0):
    rng = np.random.default_rng([seed, H, W, CS])
    bias = (1.0 + 0.2 * rng.random(H * W)).astype(np.float32)
    basis = (0.05 * rng.standard_normal((H * W, CS))).astype(np.float32)
    code = (0.3 * rng.standard_normal(CS)).astype(np.float32)
    return bias, basis, code, 1.37


def pyramid_mask(kind, H, W, seed=0):
    if kind == "ones":
        return np.ones((H, W), np.float32)
    if kind == "zeros":
        return np.zeros((H, W), np.float32)
    m = np.zeros((H, W), np.float32)
    m[2:H - 2, 2:W - 2] = 1                        # the video mask of synth.make_window
    if kind == "synthetic":
        return m
    assert kind == "holey"
    rng = np.random.default_rng([seed, H, W])
    m = np.ones((H, W), np.float32) * (rng.uniform(size=(H, W)) < 0.8)
    m[H // 4:H // 4 + 10, W // 4:W // 4 + 12] = 0  # a dead rectangle: level-1 and level-2 texels without a live tap
    return m.astype(np.float32)


def pyramid_feat(H, W, FS, seed=0):
    return np.random.default_rng([seed, H, W, FS]).uniform(-1, 1, (FS, H, W)).astype(np.float32)


def mask_levels(mask, L):
    """the mask pyramid: nearest-neighbour decimation (source index 2 i), cropped to floor(size / 2)"""
    out = [np.ascontiguousarray(mask, np.float32)]
    for _ in range(1, L):
        m = out[-1]
        out.append(np.ascontiguousarray(m[::2, ::2][:m.shape[0] // 2, :m.shape[1] // 2]))
    return out


def live_taps(mask):
    """per texel of the NEXT level: how many of its (up to nine, in-image) mask taps are nonzero, and how many exist"""
    H, W = mask.shape
    p = np.pad(mask != 0, 1).astype(np.int64)
    inside = np.pad(np.ones((H, W), np.int64), 1)
    h2, w2 = H // 2, W // 2
    live = np.zeros((h2, w2), np.int64); have = np.zeros((h2, w2), np.int64)
    for dy in range(3):
        for dx in range(3):
            live += p[dy:dy + 2 * h2:2, dx:dx + 2 * w2:2]
            have += inside[dy:dy + 2 * h2:2, dx:dx + 2 * w2:2]
    return live, have


def location_mask(kind, H, W, seed=0):
    rng = np.random.default_rng([seed, H, W])
    HW = H * W
    m = np.zeros(HW, np.float32)
    if kind == "ones":
        m[:] = 1
    elif kind == "random":
        m = (rng.random(HW) > 0.3).astype(np.float32)
    elif kind == "last_pixel":
        m[-1] = 1
    elif kind == "last_chunk":
        m[(HW - 1) // CHUNK * CHUNK:] = 1
    elif kind == "threshold":
        m = rng.random(HW).astype(np.float32)
        half = np.float32(0.5)
        m[::5] = half                                           # not > 0.5
        m[1::5] = np.nextafter(half, np.float32(1))             # the first value above
        m[2::5] = np.nextafter(half, np.float32(0))
        m[-1] = np.nextafter(half, np.float32(1))
    else:
        assert kind == "zeros"
    return m.reshape(H, W)


def location_camera(H, W):
    return synth.Camera(*[np.float32(v) for v in (0.9 * W, 0.88 * W, 0.5 * W - 0.5, 0.5 * H - 0.5, W, H)])
