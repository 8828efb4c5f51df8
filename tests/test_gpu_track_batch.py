"""sage_track_frame_batch and sage_loop_verify on the device.

The contract of the batch is BIT-EQUALITY with the single call: row b of a batch -- pose, scale, error, iterations, status
and every trace entry -- equals sage_track_frame on problem b byte for byte, for every B, every order of the problems and
whatever the other problems of the batch do (the kernels share the single call's per-pixel body and keypoint contraction and
sum a problem's per-tile records in tile order).  The problems of one batch differ in N (1, 255, 256, 257, 700: one pixel,
the tile boundary, a ragged last tile: three tiles), in NK (1, 64, 65, 160), in scene (seed) and in start, so the rounds mix linearize and
error requests and problems drop out one after the other.  Compositions: dof 6 photo + reprojection, dof 7 photo + match
geometry, photo only, keypoints only; FS = 16 and 32.  Shapes: tests/edge_scenes.LM_SCENE (32 x 40, L = 2).

sage_loop_verify: synthetic pre-check inputs at 32 x 40, C = 16, K = 64, B = 4 (synth.make_loop_candidates on a 2-pixel
grid) run through the real sage_loop_precheck; the photometric side is the LM scene's arrays under the candidates' camera (the
test is about the composition: gathered arrays exactly numpy's, every result field equal to sage_track_frame +
sage_track_overlap on the gathered inputs byte for byte)."""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import edge_scenes as es
from tests import track_batch_cases as tb
from tests.helpers import rel

pytestmark = pytest.mark.gpu

SHAPE = dict(H=32, W=40, L=2)
NS = [257, 1, 255, 256, 700]           # per problem of a batch of five
NKS = [65, 1, 64, 160, 65]
MULTIPLES = [1, "converged", 1.5, -1, 2]   # starts: multiples of the LM_START offset
SEEDS = [38, 39, 40, 41, 42]
SAMPLES = 384                          # what a 32 x 40 scene has (synth.make_window gives no more at this size)


@pytest.fixture(scope="module")
def capi():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from sage_slam_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def ws(capi):
    w = capi.Workspace()
    yield w
    w.close()


def make_scene(capi, orc, ws, **kw):
    """tests.test_gpu_tracker.Scene on the SHARED workspace (the problems of a batch must share one)"""
    from tests.test_gpu_tracker import Scene
    s = Scene(capi, orc, **kw)
    s.ws.close()
    s.ws = ws
    return s


@pytest.fixture(scope="module")
def scenes(capi, orc, ws):
    """FS -> five scenes of different seeds, 384 samples and 160 keypoints each (sized_problem makes the problems of them)"""
    return {FS: [make_scene(capi, orc, ws, seed=sd, FS=FS, n_samples=SAMPLES, NK=160, **SHAPE) for sd in SEEDS] for FS in (32, 16)}


@pytest.fixture(scope="module")
def lm_scene(capi, orc, ws):
    return make_scene(capi, orc, ws, **es.LM_SCENE)


def sized_problem(scene, dof, use_photo, use_kp, n, nk, keep):
    """the scene's problem on n samples and its first nk keypoints.  A 32 x 40 scene has at most 384 samples: sample i of the
    problem is sample i % (what the scene has) of the scene (700 of them: the scene's, then the first 316 again), every per-sample array gathered
    anew -- the pre-sampled features are [L, N, FS]"""
    import torch
    have = scene.a.homo.shape[0]
    assert nk <= scene.NK
    idx = torch.arange(n, device="cuda") % have
    d = scene.dev
    arrays = dict(homo=d["homo"][idx].contiguous(), dpts=(d["unscaled"] if dof == 7 else d["metric"])[idx].contiguous(),
                  f0s=d["f0s"][:, idx].contiguous())
    assert arrays["homo"].shape == (n, 3) and arrays["dpts"].shape == (n,) and arrays["f0s"].shape == (scene.w.L, n, scene.w.FS)
    keep.append(arrays)
    p = scene.problem(dof, use_photo, use_kp)
    p.homo_dev = arrays["homo"].data_ptr(); p.dpts0_dev = arrays["dpts"].data_ptr(); p.feat0s_dev = arrays["f0s"].data_ptr()
    p.N, p.NK = n, nk
    return p


def start_of(scene, dof, k):
    low = np.float32(float(scene.s_true) * (0.96 if dof == 7 else 1.0))
    if k == "converged":
        return scene.start_pose((0, 0, 0), (0, 0, 0)), np.float32(scene.s_true)
    return scene.start_pose(tuple(k * np.array(es.LM_START["rot"])), tuple(k * np.array(es.LM_START["trans"]))), low


def run_singles(capi, cfg, dof, probs, starts):
    out = []
    for p, (pose, s) in zip(probs, starts):
        rc, ph, sh, eh, it, tr = capi.track_frame(cfg, dof, p, pose, float(s))
        assert rc in (0, -5)
        out.append((rc, ph, np.float32(sh), np.float32(eh), it, tr))
    return out


def run_batch(capi, cfg, dof, probs, starts, idx):
    rc, P, S, E, IT, ST, TR = capi.track_frame_batch(cfg, dof, [probs[i] for i in idx], [starts[i][0] for i in idx],
                                                     [starts[i][1] for i in idx])
    assert rc == 0
    return [(ST[k], P[k], S[k], E[k], IT[k], TR[k]) for k in range(len(idx))]


def check_batches(capi, cfg, dof, probs, starts, singles, subsets):
    for idx in subsets:
        rows = run_batch(capi, cfg, dof, probs, starts, idx)
        for k, i in enumerate(idx):
            tb.assert_row_equals_single(rows[k], singles[i], f"batch {idx}, problem {i}")


SUBSETS = [[2], [3, 1], [0, 1, 2, 3, 4], [4, 2, 0, 3, 1]]       # B = 1, 2, 5 and the five permuted


@pytest.mark.parametrize("dof,use_photo,use_kp,FS", [(6, True, True, 32), (7, True, True, 32), (7, True, False, 32), (7, False, True, 32),
                                                     (7, True, True, 16), (6, True, True, 16)],
                         ids=["dof6_photo+reproj_FS32", "dof7_photo+matchgeom_FS32", "dof7_photo_FS32", "dof7_matchgeom", "dof7_photo+matchgeom_FS16",
                              "dof6_photo+reproj_FS16"])
def test_batch_rows_equal_the_single_calls_bit_for_bit(capi, scenes, dof, use_photo, use_kp, FS):
    keep = []
    cfg = capi.lm_config_default()
    probs = [sized_problem(s, dof, use_photo, use_kp, n, nk, keep) for s, n, nk in zip(scenes[FS], NS, NKS)]
    starts = [start_of(s, dof, k) for s, k in zip(scenes[FS], MULTIPLES)]
    singles = run_singles(capi, cfg, dof, probs, starts)
    print("iterations", [r[4] for r in singles])
    assert len({r[4] for r in singles}) >= 2                    # (the rounds of the batch do thin out)
    check_batches(capi, cfg, dof, probs, starts, singles, SUBSETS)


@pytest.mark.parametrize("capped", [False, True], ids=["default", "max_num_iters=2"])
@pytest.mark.parametrize("dof,use_photo,use_kp", tb.COMPOSITIONS, ids=tb.COMPOSITION_IDS)
def test_mixed_batch_of_the_cpu_test(capi, lm_scene, dof, use_photo, use_kp, capped):
    """early finisher, no_overlap exit, max_damp, iteration cap: tests/track_batch_cases.py"""
    cfg = tb.configure(capi, lm_scene, dof, use_photo, use_kp, capped)
    starts = tb.starts(lm_scene, dof, use_photo, use_kp)
    probs = [lm_scene.problem(dof, use_photo, use_kp) for _ in starts]
    singles = run_singles(capi, cfg, dof, probs, starts)
    print("iterations", [r[4] for r in singles], "status", [r[0] for r in singles])
    if dof == 7 and not use_kp:
        assert singles[3][0] == -5 and singles[3][4] == 0 and np.array_equal(singles[3][1], starts[3][0])
    if capped:
        assert max(r[4] for r in singles) == tb.CAP
    else:
        assert len({r[4] for r in singles}) >= 3 and any(not t["accepted"] for r in singles for t in r[5])
    check_batches(capi, cfg, dof, probs, starts, singles, [[0, 1, 2, 3, 4], [3, 1, 4, 0, 2]])


def test_problems_do_not_read_each_other(capi, scenes):
    """a problem with an all-zero mask (zero inliers: the 10 * sum(w) fallback and a zero system) and one with every depth
    negative next to three ordinary ones: every row is its single call's"""
    import torch
    keep = []
    dof, cfg = 7, capi.lm_config_default()
    sc = scenes[32]
    probs = [sized_problem(s, dof, True, True, n, nk, keep) for s, n, nk in zip(sc, NS, NKS)]
    starts = [start_of(s, dof, 1) for s in sc]
    zero_mask = torch.zeros_like(sc[1].dev["mask"])
    neg = -sc[3].dev["unscaled"][:256].contiguous()
    keep += [zero_mask, neg]
    probs[1] = sized_problem(sc[1], dof, True, True, 257, 65, keep)
    probs[1].mask1_dev = zero_mask.data_ptr()
    probs[3].dpts0_dev = neg.data_ptr()
    singles = run_singles(capi, cfg, dof, probs, starts)
    photo_only = capi.track_frame(cfg, dof, _photo_only(probs[1]), starts[1][0], float(starts[1][1]))
    assert photo_only[3] == pytest.approx(10.0 * float(np.sum(sc[1].w.photo_weights)))       # the fallback value is what it saw
    check_batches(capi, cfg, dof, probs, starts, singles, [[0, 1, 2, 3, 4], [0, 2, 4], [1, 3]])


def _photo_only(p):
    q = type(p).from_buffer_copy(p)
    q.use_keypoints = 0
    return q


def test_batch_against_the_oracle(capi, lm_scene):
    """dof 7 photo + match geometry, three starts whose oracle runs have no decision near a tie (asserted): the tolerances of
    tests/test_gpu_tracker.py::test_track_frame_matches_oracle_wired_lm"""
    scene, dof = lm_scene, 7
    cfg = capi.lm_config_default()
    starts = [start_of(scene, dof, k) for k in (1, -1, 1.25)]
    want = []
    for pose, s in starts:
        lin, err, decisions = es.recording_callbacks(*scene.oracle_callbacks(dof, True, True))
        po, so, eo, ito, tro = capi.track_lm(cfg, dof, lin, err, pose, float(s))
        assert es.decided_iterations(decisions, ito) == ito
        want.append((po, so, eo, ito, tro))
    rows = run_batch(capi, cfg, dof, [scene.problem(dof, True, True)] * 3, starts, [0, 1, 2])
    for (st, ph, sh, eh, ith, trh), (po, so, eo, ito, tro) in zip(rows, want):
        assert st == 0 and ith == ito and len(trh) == len(tro)
        assert [t["accepted"] for t in trh] == [t["accepted"] for t in tro]
        assert [t["relinearized"] for t in trh] == [t["relinearized"] for t in tro]
        np.testing.assert_allclose([t["error"] for t in trh], [t["error"] for t in tro], rtol=2e-4)
        np.testing.assert_allclose([t["candidate_error"] for t in trh], [t["candidate_error"] for t in tro], rtol=2e-4)
        assert float(eh) == pytest.approx(eo, rel=1e-3)
        assert rel(ph, po) < 1e-4
        assert float(sh) == pytest.approx(so, rel=1e-4)


def test_two_calls_return_identical_bytes(capi, scenes):
    keep = []
    dof, cfg = 7, capi.lm_config_default()
    probs = [sized_problem(s, dof, True, True, n, nk, keep) for s, n, nk in zip(scenes[16], NS, NKS)]
    starts = [start_of(s, dof, k) for s, k in zip(scenes[16], MULTIPLES)]
    a = run_batch(capi, cfg, dof, probs, starts, [0, 1, 2, 3, 4])
    b = run_batch(capi, cfg, dof, probs, starts, [0, 1, 2, 3, 4])
    for ra, rb in zip(a, b):
        tb.assert_row_equals_single(ra, rb)


def test_large_keypoint_sets_take_the_single_calls_launches(capi, orc, ws):
    """NK = 600 at dof 7 is past one workgroup's LDS (the batch's budget and the single call's): the problem goes through the
    single call's launches inside the round, next to one that stays on the batched launch"""
    big = make_scene(capi, orc, ws, seed=43, NK=600, n_samples=257, FS=32, **SHAPE)
    cfg = capi.lm_config_default()
    keep = []
    probs = [big.problem(7, True, True), sized_problem(big, 7, True, True, 257, 64, keep)]
    starts = [start_of(big, 7, 1), start_of(big, 7, -1)]
    singles = run_singles(capi, cfg, 7, probs, starts)
    check_batches(capi, cfg, 7, probs, starts, singles, [[0, 1], [1, 0]])


# ---------------------------------------------------------------------------------------------------------------------
# sage_loop_verify
# ---------------------------------------------------------------------------------------------------------------------
CYC_THRESH, MULT, MG_WEIGHT, DIVISOR = 1.0, 2.0, 3.0, 1.25


@pytest.fixture(scope="module")
def loop(capi, orc, ws, lm_scene):
    """pre-check outputs of four candidates (planted, self, unrelated, planted) as ctypes / cuda arrays, and the query"""
    import torch
    sc = synth.make_loop_candidates(3, 4, H=32, W=40, C=16, K=64, grid=2)
    assert [c["kind"] for c in sc["cands"]] == ["planted", "self", "unrelated", "planted"]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, K, cam = 4, sc["K"], sc["cam"]
    cands = [{k: cu(c[k]) for k in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")} for c in sc["cands"]]
    arr = (capi.SageLoopCandidate * B)(*[capi.SageLoopCandidate(*[capi.dptr(c[n]).value for n in ("desc", "dpt_map", "kp_loc", "kp_dpts0",
                                                                                                "kp_homo0")]) for c in cands])
    ccam = capi.SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    prm = capi.registration_params(synth.registration_params(1.0))
    pre = (capi.SageLoopPrecheckResult * B)()
    raw = torch.zeros(B, K, dtype=torch.int64, device="cuda")
    flags = torch.zeros(B, K, dtype=torch.int32, device="cuda")
    ikp = torch.zeros(B, K, dtype=torch.int32, device="cuda")
    desc_q = cu(sc["desc_q"])
    rc = capi.loop_precheck_raw(ws.h, capi.dptr(desc_q), DIVISOR, C.addressof(arr), B, K, 16, 32, 40, C.addressof(ccam), CYC_THRESH, MULT,
                                0.3, C.addressof(prm), C.addressof(pre), capi.dptr(raw), capi.dptr(flags), capi.dptr(ikp))
    assert rc == 0
    # arranged: candidate 2 is pruned by the ratio; candidate 1 (the query itself) is cut to three registration inliers
    assert pre[2].registered == 0 and all(pre[b].registered == 1 and pre[b].reg.n_inliers > 3 for b in (0, 1, 3))
    pre[1].reg.n_inliers = 3
    # the query's photometric side: the LM scene's arrays under the candidates' camera
    s = lm_scene
    q = capi.SageLoopVerifyQuery()
    q.N = s.a.homo.shape[0]; q.FS = s.w.FS
    q.homo_dev = s.dev["homo"].data_ptr(); q.unscaled_dpts0_dev = s.dev["unscaled"].data_ptr()
    q.feat0s_dev = s.dev["f0s"].data_ptr(); q.weights_dev = s.dev["wts"].data_ptr()
    q.pyr = capi.make_pyramid(cam, s.w.L); q.eps = s.w.eps
    assert q.pyr.P == s.pyr.P
    vy, vx = np.nonzero(s.w.mask > 0.5)
    vhomo = np.stack([(vx - cam.cx) / cam.fx, (vy - cam.cy) / cam.fy, np.ones(vx.size)], 1).astype(np.float32)
    vd = (np.float32(DIVISOR) * (s.a.bias + s.a.basis @ s.a.code_true)[vy * 40 + vx]).astype(np.float32)
    dev = dict(vhomo=cu(vhomo), vd=cu(vd))
    q.M = vx.size; q.valid_homo_dev = dev["vhomo"].data_ptr(); q.valid_dpts0_dev = dev["vd"].data_ptr()
    q.mask_dev = s.dev["mask"].data_ptr()
    vcands = [dict(feat1=s.dev["feat1"], grad1=s.dev["grad1"], mask1=s.dev["mask"], kp_loss_param=s.mg_loss_param * (1 + 0.1 * b))
              for b in range(B)]
    return dict(sc=sc, cands=cands, arr=arr, pre=pre, raw=raw, ikp=ikp, q=q, vcands=vcands, dev=dev, cam=cam, K=K, B=B, desc_q=desc_q)


def test_loop_verify_equals_its_single_call_composition(capi, ws, lm_scene, loop):
    import torch
    F = np.float32
    L, K, cam, q = loop, loop["K"], loop["cam"], loop["q"]
    cfg = capi.lm_config_default()
    cfg.no_overlap_error = 1e-3                                       # (must not be read: the match-geometry term is on)
    res, gathered = capi.loop_verify(ws, cfg, q, DIVISOR, L["cands"], L["vcands"], L["pre"], L["raw"], L["ikp"], MG_WEIGHT)
    g = gathered.cpu().numpy()
    survivors = [b for b in range(4) if L["pre"][b].registered == 1 and L["pre"][b].reg.n_inliers > 3]
    assert survivors == [0, 3]
    for b in (1, 2):                                                  # <= 3 inliers; pruned: not tracked, nothing gathered
        assert res[b].tracked == 0 and res[b].iters == 0 and res[b].scale == 0 and not g[b].any()
    raw, ikp = L["raw"].cpu().numpy(), L["ikp"].cpu().numpy()
    cfg1 = capi.lm_config_default()
    for b in survivors:
        pre = L["pre"][b]
        n = pre.reg.n_inliers
        i = ikp[b, :n]
        c = L["sc"]["cands"][b]
        # the gather: integer gathers and single fp32 operations -> exactly numpy's
        loc = raw[b, i]
        lf = loc.astype(F)
        homo1 = np.stack([(np.fmod(lf, F(40)) - F(cam.cx)) / F(cam.fx), (np.floor(lf / F(40)) - F(cam.cy)) / F(cam.fy), np.ones(n, F)], 1)
        want = dict(homo0=c["kp_homo0"][i], dpts0=c["kp_dpts0"][i] / F(DIVISOR), homo1=homo1.astype(F), dpts1=c["dpt_map"][loc])
        got = dict(homo0=g[b, :3 * K].reshape(K, 3)[:n], dpts0=g[b, 3 * K:4 * K][:n], homo1=g[b, 4 * K:7 * K].reshape(K, 3)[:n],
                   dpts1=g[b, 7 * K:8 * K][:n])
        for k in want:
            assert want[k].dtype == F and got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), (b, k)
        # the composition: sage_track_frame on the gathered inputs, then sage_track_overlap
        p = capi.SageTrackProblem()
        p.ws = ws.h; p.use_photo = 1; p.use_keypoints = 1
        v = L["vcands"][b]
        p.mask1_dev = v["mask1"].data_ptr(); p.feat1_dev = v["feat1"].data_ptr(); p.grad1_dev = v["grad1"].data_ptr()
        p.dpts0_dev = q.unscaled_dpts0_dev; p.homo_dev = q.homo_dev; p.feat0s_dev = q.feat0s_dev; p.weights_dev = q.weights_dev
        p.pyr = q.pyr; p.eps = q.eps; p.N = q.N; p.FS = q.FS; p.NK = n
        base = gathered.data_ptr() + b * 8 * K * 4
        p.kp_homo0_dev = base; p.kp_dpts0_dev = base + 3 * K * 4; p.kp_matched_homo1_dev = base + 4 * K * 4
        p.kp_matched_dpts1_dev = base + 7 * K * 4
        p.kp_loss_param = v["kp_loss_param"]
        p.kp_weight = float(F(pre.desc_match_inlier_ratio) * F(MG_WEIGHT))
        pose0 = np.concatenate([np.array(pre.reg.R[:], np.float64), np.array(pre.reg.t[:], np.float64)]).astype(F)
        rc, ph, sh, eh, it, _ = capi.track_frame(cfg1, 7, p, pose0, float(F(pre.reg.scale)))
        r = res[b]
        assert rc == 0 and r.tracked == 1 and r.status == 0 and r.iters == it and it >= 1
        assert np.array(r.pose12[:], F).tobytes() == ph.tobytes()
        assert F(r.scale).tobytes() == F(sh).tobytes() and F(r.error).tobytes() == F(eh).tobytes()
        ov = capi.track_overlap(ws, ph[:9], ph[9:], L["dev"]["vd"], L["dev"]["vhomo"], cam, lm_scene.dev["mask"], q.eps,
                                depth_scale=float(F(sh) / F(DIVISOR)))
        for k in ("area_ratio", "inlier_ratio", "average_motion"):
            assert F(getattr(r, k)).tobytes() == F(getattr(ov, k)).tobytes(), k
        assert F(r.area_inlier_ratio).tobytes() == (F(ov.area_ratio) * F(ov.inlier_ratio)).tobytes()
    # determinism
    res2, gathered2 = capi.loop_verify(ws, cfg, q, DIVISOR, L["cands"], L["vcands"], L["pre"], L["raw"], L["ikp"], MG_WEIGHT)
    assert bytes(res2) == bytes(res) and torch.equal(gathered2, gathered)


def test_loop_verify_without_survivors_launches_nothing(capi, ws, loop):
    """no survivor: the results are zeroed and the gathered array is not touched"""
    import torch
    L = loop
    pre = (capi.SageLoopPrecheckResult * 4).from_buffer_copy(L["pre"])
    for b in range(4):
        pre[b].reg.n_inliers = min(pre[b].reg.n_inliers, 3)
    gathered = torch.full((4, 8 * L["K"]), 7.0, dtype=torch.float32, device="cuda")
    res = (capi.SageLoopVerifyResult * 4)()
    for r in res:
        r.tracked = 77
    cfg = capi.lm_config_default()
    arr = L["arr"]
    varr = (capi.SageLoopVerifyCandidate * 4)(*[capi.SageLoopVerifyCandidate(v["feat1"].data_ptr(), v["grad1"].data_ptr(), v["mask1"].data_ptr(),
                                                                             v["kp_loss_param"]) for v in L["vcands"]])
    args = lambda **kw: [kw.get("ws", ws.h), C.addressof(cfg), C.addressof(L["q"]), kw.get("divisor", DIVISOR), C.addressof(arr),
                         C.addressof(varr), C.addressof(pre), 4, L["K"], capi.dptr(L["raw"]), capi.dptr(L["ikp"]), MG_WEIGHT,
                         kw.get("gathered", capi.dptr(gathered)), C.addressof(res)]
    assert capi.loop_verify_raw(*args()) == 0
    torch.cuda.synchronize()
    assert all(r.tracked == 0 for r in res) and bool((gathered == 7.0).all())
    # invalid arguments answer before any launch
    for r in res:
        r.tracked = 77
    for kw in (dict(ws=None), dict(divisor=0.0), dict(gathered=None)):
        assert capi.loop_verify_raw(*args(**kw)) == -1
    torch.cuda.synchronize()
    assert all(r.tracked == 77 for r in res) and bool((gathered == 7.0).all())
