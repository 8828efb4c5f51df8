"""One long-lived SageWorkspace against fresh ones, bit for bit: what a workspace keeps between calls -- the cached work list
(dense or tracker, for one N), its pinned regions (operator statistics, tracker evaluation, overlap survivors) and where an
operator's statistics go -- must never reach a result.  Every call is repeated on a workspace of its own and compared as bytes.

Inputs: the tracker scene of tests/test_gpu_tracker.py (64x80, its first N samples) and the 48x64 overlap case "small"."""
import numpy as np
import pytest

from sage_slam_amd import synth
from tests.test_gpu_track_overlap import case, raw, run
from tests.test_gpu_tracker import Scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def scene(capi, orc):
    s = Scene(capi, orc)
    yield s
    s.close()


def as_bytes(r):
    """an operator's result -- a dict of arrays and floats, or a tuple of floats -- as bytes"""
    if isinstance(r, dict):
        return b"".join(as_bytes(r[k]) for k in sorted(r))
    if isinstance(r, (tuple, list)):
        return b"".join(as_bytes(v) for v in r)
    return np.asarray(r, np.float32).tobytes()


def on_fresh(capi, call):
    ws = capi.Workspace()
    try:
        return call(ws)
    finally:
        ws.close()


class Ops:
    """the per-edge operators on the first N samples of the scene's edge 0 -> 1, each as a function of the workspace"""

    def __init__(self, capi, scene):
        import torch
        self.capi, self.s = capi, scene
        w, a, b = scene.w, scene.a, scene.b
        self.A, self.B = capi.DeviceKeyframe(a, w.H, w.W), capi.DeviceKeyframe(b, w.H, w.W)
        self.R10, self.t10 = synth.relative_pose(a.R, a.t, b.R, b.t)
        self.dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        ws = capi.Workspace()
        self.dpt1, _ = capi.depth_and_grad(ws, self.B.bias, self.B.basis, b.code, b.scale, w.H, w.W, w.CS)
        ws.close()

    def photo_jac(self, N):
        c, s, A, B = self.capi, self.s, self.A, self.B
        w, a, b = s.w, s.a, s.b
        return lambda ws: c.photometric_jac_error(ws, self.R10, self.t10, a.R, a.t, b.R, b.t, A.bias, A.basis, a.code, s.dev["mask"],
                                                  A.loc1d[:N], A.homo[:N], A.feat_pyr, B.feat_pyr, B.grad_pyr, a.scale, s.pyr,
                                                  w.eps, w.photo_weights, w.FS, w.CS)

    def photo_err(self, N):
        c, s, A, B = self.capi, self.s, self.A, self.B
        w, a = s.w, s.a
        return lambda ws: c.photometric_error(ws, self.R10, self.t10, A.bias, A.basis, a.code, s.dev["mask"], A.loc1d[:N],
                                              A.homo[:N], A.feat_pyr, B.feat_pyr, a.scale, s.pyr, w.eps, w.photo_weights, w.FS,
                                              w.CS)

    def geo_err(self, N):
        c, s, A = self.capi, self.s, self.A
        w, a = s.w, s.a
        return lambda ws: c.geometric_error(ws, self.R10, self.t10, A.bias, A.basis, a.code, self.dpt1, s.dev["mask"],
                                            A.loc1d_i32[:N], A.homo[:N], a.scale, s.pyr.cam[0], w.eps, w.geo_loss_param,
                                            w.geo_weight, w.CS)

    def track_args(self, N):
        s, d = self.s, self.s.dev
        p = s.start_pose()
        return p[:9], p[9:], d["mask"], d["metric"][:N].contiguous(), d["homo"][:N].contiguous(), d["f0s"][:, :N].contiguous()

    def track_jac(self, N):
        c, s, d = self.capi, self.s, self.s.dev
        R, t, mask, dpts, homo, f0s = self.track_args(N)
        return lambda ws: c.tracker_photo_jac_error(ws, 6, R, t, mask, dpts, homo, f0s, d["feat1"], d["grad1"], s.pyr, 1.0,
                                                    s.w.eps, d["wts"], s.w.FS)

    def track_err(self, N):
        c, s, d = self.capi, self.s, self.s.dev
        R, t, mask, dpts, homo, f0s = self.track_args(N)
        return lambda ws: c.tracker_photo_error(ws, R, t, mask, dpts, homo, f0s, d["feat1"], s.pyr, s.w.eps, d["wts"], s.w.FS)

    def track_reproj_err(self):
        c, s, d = self.capi, self.s, self.s.dev
        p = s.start_pose()
        R, t = self.dv(p[:9]), self.dv(p[9:])
        return lambda ws: c.tracker_reproj_error(ws, R, t, d["kp_metric"], d["kp_homo0"], d["kp_2d"], s.pyr.cam[0], s.w.eps,
                                                 s.reproj_loss_param, s.reproj_weight)


def test_work_list_cache_across_kinds(capi, scene):
    """a dense list and a tracker list of the SAME N = 257 (two tiles, the second with one pixel) follow each other, then
    other N of either kind: no call may run on the list the call before it left behind"""
    ops = Ops(capi, scene)
    seq = [("dense photometric linearize, N 257", ops.photo_jac(257)), ("tracker photometric linearize, N 257", ops.track_jac(257)),
           ("dense photometric linearize, N 257 again", ops.photo_jac(257)), ("geometric error, N 256", ops.geo_err(256)),
           ("tracker photometric error, N 1", ops.track_err(1)), ("dense photometric error, N 256", ops.photo_err(256))]
    ws = capi.Workspace()
    try:
        for what, call in seq:
            got, want = call(ws), on_fresh(capi, call)
            err = got["error"] if isinstance(got, dict) else got[0]
            print(f"{what}: error {err!r}")
            assert np.isfinite(err) and err > 0, what
            assert as_bytes(got) == as_bytes(want), what
    finally:
        ws.close()


def test_overlap_region_grows_and_is_reused(capi, scene):
    """sage_track_overlap with M = 300, then 2176, then 300 again on one workspace: the pinned region grows, then holds a
    smaller problem than it has room for; a tracked frame between the calls gives the same result every time"""
    prob = case("small")[0]
    few = {**prob, "dpts0": prob["dpts0"][:300], "homo": prob["homo"][:300], "M": 300}
    cfg = capi.lm_config_default()
    cfg.max_num_iters = 3
    tprob = scene.problem(6, True, True)
    frame = lambda: capi.track_frame(cfg, 6, tprob, scene.start_pose(), 1.0)
    frames = [frame()]
    for p in (few, prob, few):
        got, want = run(capi, scene.ws, p), on_fresh(capi, lambda ws: run(capi, ws, p))
        print(f"M {p['M']}: candidates {list(got.n_candidates)} area_ratio {got.area_ratio!r}")
        assert got.n_points == p["M"] and got.n_candidates[0] > 0
        assert raw(got) == raw(want)
        frames.append(frame())
    for f in frames:
        assert f[0] == 0
        assert f[1].tobytes() == frames[0][1].tobytes() and f[2:] == frames[0][2:]


def test_a_tracked_frame_leaves_no_mode_behind(capi, scene):
    """after a rejected sage_track_frame and after one that ends normally, the public operators on the same workspace hand
    their statistics to the caller as on a fresh workspace"""
    ops = Ops(capi, scene)
    cfg = capi.lm_config_default()
    cfg.max_num_iters = 3
    checks = [("photometric error", ops.photo_err(256)), ("tracker reprojection error", ops.track_reproj_err())]
    want = [on_fresh(capi, call) for _, call in checks]
    rejected = capi.track_frame(cfg, 7, scene.problem(7, False, False), scene.start_pose(), 1.0)
    assert rejected[0] == -1
    for (what, call), w in zip(checks, want):
        assert as_bytes(call(scene.ws)) == as_bytes(w), what + " after a rejected frame"
    done = capi.track_frame(cfg, 6, scene.problem(6, True, True), scene.start_pose(), 1.0)
    assert done[0] == 0
    for (what, call), w in zip(checks, want):
        got = call(scene.ws)
        print(f"{what}: error {got[0]!r} inliers {got[1]!r}")
        assert got[0] > 0 and got[1] > 0
        assert as_bytes(got) == as_bytes(w), what + " after a tracked frame"
