"""The front-end tracker's photometric kernels (track_kernels.hip: track_kernel<16 / 32, JAC>, track_finalize_kernel)
at their edge shapes, through the operators sage_tracker_photo_jac_error_calculate / sage_tracker_photo_error_calculate,
against the fp64 oracle.

Cases (tests/edge_scenes.TRACKER_CASES, dof 6 and 7 each): FS = 32 on 32x40 with L = 2 at N = 1, 2, 63, 64, 65, 255, 256,
257 -- below a wave, a full wave, one lane into the next wave, one lane short of a 256-sample tile, a full tile, one
sample in a second tile; FS = 16 on 64x80 with L = 4 at N = 65, 257, 513, 700; FS = 32 at N = 700; L = 1; the non-dyadic
pyramid 50x62 -> 25x31 -> 12x15, dense, at FS = 32.  Every scene has about 20 % holes in the destination mask and every
7th source depth negative: mixed validity inside every wave.  tests/test_edge_scenes.py shows on the CPU that each case
has 0 < inliers < N (N = 1: its one inlier), that the LAST sample is an inlier, and that the oracle's AtA without it is
100 bars away (the dense case: without its partial last tile of 32 samples -- no single one of its 1460 inliers carries
100 bars, the last one carries 20): a dead tail lane that leaks in, a lost tail lane or a lost last tile cannot pass.

Bars.  Inlier count: exact.  AtA, Atb: rel-L2 against the fp64 oracle below max(2e-5, 4 x the fp32 oracle's own rel-L2
distance from fp64 on the case); error: relative, below max(1e-5, 4 x the fp32 oracle's).  2e-5 / 1e-5 are the project's
bars (tests/test_gpu_parity.py); the kernel sums in another order with contracted multiply-adds, so it gets those or
four times the reference's own rounding, whichever is larger.  A wrong tap, weight or lane moves these by 1e-3 or more.
Next to them, entry by entry: dist_A / dist_b of tests/system_metric.py against the fp64 oracle under the bars of the
"tracker_photometric" family (D = 6 and D = 7: the 7-dof scale row is small next to the pose rows in the norms above).

Measured on an MI355X: the kernel's distance from the fp64 oracle as a share of its bar, the worse of dof 6 and 7
(the bar was the project's 2e-5 / 1e-5 on every case: the fp32 oracle is 1e-8 .. 2e-6 from fp64 here)

  case                       AtA     Atb     error   error-only
  32x40_FS32_L2_N1           0.008   0.015   0.028   0.039
  32x40_FS32_L2_N2           0.009   0.079   0.217   0.217
  32x40_FS32_L2_N63          0.004   0.045   0.129   0.129
  32x40_FS32_L2_N64          0.003   0.003   0.013   0.013
  32x40_FS32_L2_N65          0.003   0.006   0.009   0.019
  32x40_FS32_L2_N255         0.003   0.002   0.008   0.008
  32x40_FS32_L2_N256         0.002   0.058   0.043   0.035
  32x40_FS32_L2_N257         0.003   0.002   0.013   0.013
  64x80_FS16_L4_N65          0.007   0.035   0.060   0.060
  64x80_FS16_L4_N257         0.003   0.006   0.006   0.006
  64x80_FS16_L4_N513         0.002   0.018   0.034   0.034
  64x80_FS16_L4_N700         0.001   0.016   0.067   0.067
  64x80_FS32_L4_N700         0.004   0.043   0.059   0.059
  32x40_FS16_L1_N50          0.004   0.005   0.007   0.016
  50x62_FS32_L3_Ndense       0.004   0.023   0.030   0.039

With the last tile dropped from the finalize kernel's sum the cases N = 257, 513, 700 and the dense one fail; with the
wave sums read from lane 0 every case from N = 63 on fails (and the LM run, both times).

The zero-inlier result on the operator itself (the 32x40 scene moved 50 behind the camera): no inlier, AtA and Atb
without a nonzero element, error = 10 sum(weights) from both entry points.

One LM run at a second shape: sage_track_frame against sage_track_lm over the oracle's kernels on the 32x40, FS = 32,
L = 2, N = 257, NK = 65 scene (tests/edge_scenes.LM_SCENE), dof 6 photometric + reprojection and dof 7 photometric +
match geometry, with the assertions of tests/test_gpu_tracker.py.  Every accept / reject decision of the oracle's run
is at least 1e-2 of the error away from a tie (50 x the 2e-4 the traces are compared to: fp32 noise cannot flip one),
so the whole run is compared: 4 iterations, 3 of them with a step (the fourth ends on the convergence test).
"""
import numpy as np
import pytest

from tests import edge_scenes as es
from tests import system_metric as sm
from tests.conftest import summary_line
from tests.helpers import rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module", autouse=True)
def _metric_summary():
    yield
    for ln in sm.summary_lines("tracker edge shapes"):
        summary_line(ln)


@pytest.fixture(scope="module")
def ws(capi):
    w = capi.Workspace()
    yield w
    w.close()


def _device(capi, s):
    import torch
    dv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return dict(pyr=capi.make_pyramid(s.cams[0], s.L), mask=dv(s.mask), dpts0=dv(s.dpts0), homo=dv(s.homo),
                feat0s=dv(s.feat0s), feat1=dv(s.feat1), grad1=dv(s.grad1), weights=dv(s.weights))


def _hip_jac(capi, ws, s, d, dof):
    return capi.tracker_photo_jac_error(ws, dof, s.R, s.t, d["mask"], d["dpts0"], d["homo"], d["feat0s"], d["feat1"],
                                        d["grad1"], d["pyr"], s.scale0, s.eps, d["weights"], s.FS)


def _hip_err(capi, ws, s, d):
    return capi.tracker_photo_error(ws, s.R, s.t, d["mask"], d["dpts0"], d["homo"], d["feat0s"], d["feat1"], d["pyr"],
                                    s.eps, d["weights"], s.FS)


@pytest.mark.parametrize("case", es.TRACKER_CASES, ids=es.tracker_case_id)
def test_tracker_kernels_at_edge_shapes(capi, ws, orc, case):
    s = es.tracker_scene(**case)
    d = _device(capi, s)
    worst = dict(AtA=0.0, Atb=0.0, error=0.0, error_only=0.0)
    failures = []
    for dof in (6, 7):
        o64, (e64, n64), own, bars = es.tracker_bars(orc, s, dof)
        h = _hip_jac(capi, ws, s, d, dof)
        he, hn = _hip_err(capi, ws, s, d)
        got = dict(AtA=rel(h["AtA"], o64["AtA"]), Atb=rel(h["Atb"], o64["Atb"]),
                   error=abs(h["error"] - o64["error"]) / abs(o64["error"]), error_only=abs(he - e64) / abs(e64))
        for k in worst:
            worst[k] = max(worst[k], got[k] / bars[k])
            if not got[k] < bars[k]:
                failures.append(f"dof {dof} {k}: {got[k]:.3e} against a bar of {bars[k]:.3e}")
        try:
            sm.check(h, o64, "tracker_photometric", f"{es.tracker_case_id(case)} dof {dof}")
        except AssertionError as e:
            failures.append(str(e))
        if h["num_inliers"] != o64["num_inliers"] or hn != n64:
            failures.append(f"dof {dof} inliers: {h['num_inliers']} / {hn} against {o64['num_inliers']} / {n64}")
    summary_line(f"tracker shapes {es.tracker_case_id(case):24s} share of the bar: AtA {worst['AtA']:.3f}  Atb {worst['Atb']:.3f}  "
                 f"error {worst['error']:.3f}  error-only {worst['error_only']:.3f}")
    assert not failures, failures


@pytest.mark.parametrize("dof", [6, 7])
def test_tracker_zero_inliers_on_the_operator(capi, ws, orc, dof):
    """every sample behind the camera: the finalize kernel's fallback, not a fault -- exact zeros and 10 sum(weights)"""
    s = es.tracker_scene(**es.ZERO_INLIER_CASE, far=True)
    d = _device(capi, s)
    fallback = 10.0 * float(np.sum(s.weights, dtype=np.float32))
    o = es.oracle_jac(orc, s, dof)
    assert o["num_inliers"] == 0 and o["error"] == fallback
    h = _hip_jac(capi, ws, s, d, dof)
    assert h["num_inliers"] == 0
    assert not h["AtA"].any() and not h["Atb"].any()
    assert h["error"] == fallback
    he, hn = _hip_err(capi, ws, s, d)
    assert hn == 0 and he == fallback


@pytest.fixture(scope="module")
def lm_scene(capi, orc):
    from tests.test_gpu_tracker import Scene
    s = Scene(capi, orc, **es.LM_SCENE)
    yield s
    s.close()


@pytest.mark.parametrize("dof,use_photo,use_kp", es.LM_COMPOSITIONS, ids=["new_photo+reproj", "frame_photo+matchgeom"])
def test_track_frame_matches_oracle_wired_lm_at_a_second_shape(capi, lm_scene, dof, use_photo, use_kp):
    scene = lm_scene
    cfg = capi.lm_config_default()
    pose0 = scene.start_pose(**es.LM_START)
    s0 = float(scene.s_true) * (0.96 if dof == 7 else 1.0)
    lin, err, decisions = es.recording_callbacks(*scene.oracle_callbacks(dof, use_photo, use_kp))
    po, so, eo, ito, tro = capi.track_lm(cfg, dof, lin, err, pose0, s0)
    # the precondition on the oracle's own run: no decision near a tie, so the whole run is compared
    assert es.decided_iterations(decisions, ito) == ito and len(tro) >= es.LM_MIN_ITERS
    rc, ph, sh, eh, ith, trh = capi.track_frame(cfg, dof, scene.problem(dof, use_photo, use_kp), pose0, s0)
    assert rc == 0
    summary_line(f"tracker LM 32x40 FS32 dof {dof}: iters {ith}/{ito}  error {tro[0]['error']:.5f} -> {eh:.5f}/{eo:.5f}  "
                 f"scale {s0:.5f} -> {sh:.5f}/{so:.5f}  pose rel {rel(ph, po):.1e}")
    assert ith == ito and len(trh) == len(tro)
    assert [t["accepted"] for t in trh] == [t["accepted"] for t in tro]
    assert [t["relinearized"] for t in trh] == [t["relinearized"] for t in tro]
    np.testing.assert_allclose([t["error"] for t in trh], [t["error"] for t in tro], rtol=2e-4)
    np.testing.assert_allclose([t["candidate_error"] for t in trh], [t["candidate_error"] for t in tro], rtol=2e-4)
    assert eh == pytest.approx(eo, rel=1e-3)
    assert rel(ph, po) < 1e-4
    if dof == 7:
        assert sh == pytest.approx(so, rel=1e-4)
        assert abs(sh / float(scene.s_true) - 1.0) < 0.5 * 0.04
    assert eo < 0.7 * tro[0]["error"]
    assert np.linalg.norm(ph[9:] - scene.t10) < np.linalg.norm(pose0[9:] - scene.t10)
