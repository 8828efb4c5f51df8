"""sage_loop_accept on the device.

A synthetic detector round at 48 x 64 with B = 6: `pre` and `ver` are made by hand (no tracker run), the depth-scale inputs of
candidate b are synth.make_depth_scale_problem(48, 64, "small", seed 1 + b), the keyframe to scale is that of seed 1.  The
tracked pose of candidate b is the inverse of its problem's pose, its translation times tracker_ref_scale / dpt_scale, so
the pose the library hands over is the problem's pose up to rounding; what the test compares with is the pose of
tests/loop_accept_ref.py, byte for byte, and sage_depth_scale_ratio (drop_nan = 1) on that pose.

  b   id   area  inlier  metric  desc   outcome
  0   10   0.30  0.90    0.27    0.9    fails the overlap test (area)
  1   20   0.80  0.80    0.64    0.5    accepted, kept second
  2   30   0.90  0.20    0.18    0.9    fails the overlap test (inliers)
  3   40   0.90  0.90    0.81    0.7    accepted, kept first
  4   50   0.55  0.55    0.3025  0.9    fails the base metric (0.35)
  5   43   0.70  0.80    0.56    0.6    accepted, within redundant_range (5) of id 40: dropped

A second round (TIES) accepts all six, with equal descriptor ratios and ids exactly at and just inside redundant_range:

  b   id    desc   outcome (redundant_range 5)
  0   100   0.6    kept third: ties with b4, candidate order puts it first
  1   200   0.8    kept first: ties with b2, candidate order puts it first
  2   205   0.8    kept second: |205 - 200| = 5 is not < 5
  3   204   0.7    dropped: 4 from id 200
  4   300   0.6    kept fourth
  5   295   0.5    kept fifth: exactly 5 from id 300

One more case chains sage_loop_precheck -> sage_loop_verify -> sage_loop_accept on the arrays tests/test_gpu_track_batch.py
builds for its sage_loop_verify test: the three calls hand their arrays on as they are."""
import ctypes as C

import numpy as np
import pytest

from sage_slam_amd import synth
from tests import loop_accept_ref as lref
from tests.test_gpu_track_batch import DIVISOR, MG_WEIGHT, capi, lm_scene, loop, ws  # noqa: F401  (fixtures and builders)

pytestmark = pytest.mark.gpu

F = np.float32
CFG = dict(min_area_ratio=0.5, min_inlier_ratio=0.5, base_metric=0.35, base_desc_ratio=0.2, redundant_range=5, dpt_eps=1e-4)
ROUND = [dict(id=10, area_ratio=0.30, inlier_ratio=0.90, desc=0.9), dict(id=20, area_ratio=0.80, inlier_ratio=0.80, desc=0.5),
         dict(id=30, area_ratio=0.90, inlier_ratio=0.20, desc=0.9), dict(id=40, area_ratio=0.90, inlier_ratio=0.90, desc=0.7),
         dict(id=50, area_ratio=0.55, inlier_ratio=0.55, desc=0.9), dict(id=43, area_ratio=0.70, inlier_ratio=0.80, desc=0.6)]


TIES = [dict(id=100, area_ratio=0.9, inlier_ratio=0.9, desc=0.6), dict(id=200, area_ratio=0.9, inlier_ratio=0.9, desc=0.8),
        dict(id=205, area_ratio=0.9, inlier_ratio=0.9, desc=0.8), dict(id=204, area_ratio=0.9, inlier_ratio=0.9, desc=0.7),
        dict(id=300, area_ratio=0.9, inlier_ratio=0.9, desc=0.6), dict(id=295, area_ratio=0.9, inlier_ratio=0.9, desc=0.5)]


def cu(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def raw(st):
    return bytes(memoryview(st))


def accept_cfg(capi, cfg):
    return capi.SageLoopAcceptConfig(*[cfg[k] for k, _ in capi.SageLoopAcceptConfig._fields_])


def build_round(capi, spec):
    """the candidates as tests/loop_accept_ref.py takes them, their device arrays, and the ctypes pre / ver"""
    probs = [synth.make_depth_scale_problem(48, 64, "small", 1 + b) for b in range(6)]
    cands, dcands, scands = [], [], []
    pre = (capi.SageLoopPrecheckResult * 6)()
    ver = (capi.SageLoopVerifyResult * 6)()
    for b, (c, p) in enumerate(zip(spec, probs)):
        dpt_scale, ref_scale = F(1.0 + 0.25 * b), F(0.8 + 0.1 * b)
        R, t = p["R"].astype(F), p["t"].astype(F)
        pose12 = np.concatenate([R.T.reshape(9), -(R.T @ t) * ref_scale / dpt_scale]).astype(F)
        metric = F(F(c["area_ratio"]) * F(c["inlier_ratio"]))
        cands.append(dict(c, tracked=1, status=0, area_inlier_ratio=metric, pose12=pose12, dpt_scale=dpt_scale, tracker_ref_scale=ref_scale))
        dcands.append(dict(dpt_map=cu(p["dpt0_map"].reshape(-1))))
        scands.append(dict(id=c["id"], valid_loc1d=cu(p["loc1d0"], np.int64), valid_homo=cu(p["homo"]), dpt_scale=dpt_scale,
                           tracker_ref_scale=ref_scale))
        pre[b].desc_match_inlier_ratio = c["desc"]
        v = ver[b]
        v.tracked, v.status, v.area_ratio, v.inlier_ratio, v.area_inlier_ratio = 1, 0, c["area_ratio"], c["inlier_ratio"], metric
        v.pose12[:] = [float(x) for x in pose12]
    q = probs[0]
    return dict(cands=cands, dcands=dcands, scands=scands, pre=pre, ver=ver, bias=cu(q["bias1"]), mask=cu(q["mask"]), cam=q["cam"])


@pytest.fixture(scope="module")
def round6(capi):
    return build_round(capi, ROUND)


def check_against_the_restatement(capi, ws, cfg, cands, dcands, scands, bias, mask, cam, infos, kept):
    acc, want_kept = lref.filter_kept(cfg, cands)
    assert kept == want_kept
    for b, c in enumerate(cands):
        li = infos[b]
        assert li.accepted == int(acc[b]) and li.kept == int(b in want_kept)
        if not acc[b]:
            assert raw(li) == bytes(C.sizeof(li))
            continue
        Rt, t = lref.pose(c["pose12"], c["dpt_scale"], c["tracker_ref_scale"])
        assert np.array(li.R_cur_ref[:], F).tobytes() == Rt.tobytes() and np.array(li.t_cur_ref[:], F).tobytes() == t.tobytes()
        assert li.id_ref == c["id"] and F(li.ref_scale) == F(c["dpt_scale"]) and F(li.desc_inlier_ratio) == F(c["desc"])
        assert F(li.metric) == F(c["area_inlier_ratio"])
        want = capi.depth_scale_ratio(ws, Rt, t, dcands[b]["dpt_map"], scands[b]["valid_homo"], cam, bias, mask, cfg["dpt_eps"], True,
                                      scands[b]["valid_loc1d"])
        assert raw(li.scale) == raw(want)
        assert F(li.query_scale).tobytes() == F(want.ratio).tobytes()
        print(f"candidate {b} id {c['id']}: query_scale {li.query_scale!r} used {li.scale.n_used} of {li.scale.n_points} kept {li.kept}")
    return acc, want_kept


def test_a_detector_round(capi, round6):
    r = round6
    w = capi.Workspace()
    try:
        assert capi.depth_scale_ratio_batch_launches(w) == 0
        infos, kept = capi.loop_accept(w, accept_cfg(capi, CFG), r["bias"], r["mask"], r["cam"], r["dcands"], r["scands"], r["pre"], r["ver"])
        Ms = [int(r["scands"][b]["valid_homo"].shape[0]) for b in (1, 3, 5)]
        assert capi.depth_scale_ratio_batch_launches(w) == capi.depth_scale_ratio_batch_plan(Ms)["launches"] == 5   # one batch
        acc, want_kept = check_against_the_restatement(capi, w, CFG, r["cands"], r["dcands"], r["scands"], r["bias"], r["mask"], r["cam"],
                                                       infos, kept)
    finally:
        w.close()
    assert acc == [False, True, False, True, False, True] and want_kept == [3, 1]
    assert all(np.isfinite(infos[b].query_scale) and infos[b].scale.n_used > 0 for b in (1, 3, 5))
    # the pose handed over is the problem's pose up to the rounding of the inverse and the two rescalings
    p = synth.make_depth_scale_problem(48, 64, "small", 4)
    assert np.allclose(np.array(infos[3].R_cur_ref[:]).reshape(3, 3), p["R"], atol=1e-6)
    assert np.allclose(np.array(infos[3].t_cur_ref[:]), p["t"], rtol=1e-5, atol=1e-6)


def test_ties_keep_candidate_order_and_the_range_is_exclusive(capi, ws):
    """the library's sort and filter on the hand-derived order of the module's docstring (and on the restatement's)"""
    r = build_round(capi, TIES)
    infos, kept = capi.loop_accept(ws, accept_cfg(capi, CFG), r["bias"], r["mask"], r["cam"], r["dcands"], r["scands"], r["pre"], r["ver"])
    assert kept == [1, 2, 0, 4, 5]
    assert [infos[b].accepted for b in range(6)] == [1] * 6 and [infos[b].kept for b in range(6)] == [1, 1, 1, 0, 1, 1]
    acc, want_kept = check_against_the_restatement(capi, ws, CFG, r["cands"], r["dcands"], r["scands"], r["bias"], r["mask"], r["cam"], infos,
                                                   kept)
    assert acc == [True] * 6 and want_kept == kept
    # a range of 1 drops nobody (the ids differ): the order is the sort's alone, ties in candidate order
    infos, kept = capi.loop_accept(ws, accept_cfg(capi, {**CFG, "redundant_range": 1}), r["bias"], r["mask"], r["cam"], r["dcands"],
                                   r["scands"], r["pre"], r["ver"])
    assert kept == [1, 2, 3, 0, 4, 5]
    # a range of 6 takes the pairs at 5 as well: 205 goes because of 200, 295 because of 300
    infos, kept = capi.loop_accept(ws, accept_cfg(capi, {**CFG, "redundant_range": 6}), r["bias"], r["mask"], r["cam"], r["dcands"],
                                   r["scands"], r["pre"], r["ver"])
    assert kept == [1, 0, 4]


def test_a_round_without_an_accepted_candidate_launches_nothing(capi, round6):
    r = round6
    w = capi.Workspace()
    try:
        infos, kept = capi.loop_accept(w, accept_cfg(capi, {**CFG, "base_desc_ratio": 0.95}), r["bias"], r["mask"], r["cam"], r["dcands"],
                                       r["scands"], r["pre"], r["ver"])
        assert kept == [] and all(raw(infos[b]) == bytes(C.sizeof(infos[b])) for b in range(6))
        assert capi.depth_scale_ratio_batch_launches(w) == 0
    finally:
        w.close()


def test_precheck_verify_accept_chain(capi, ws, loop):
    """the arrays of sage_loop_precheck and sage_loop_verify go into sage_loop_accept as they are"""
    L, cam = loop, loop["cam"]
    cfg = capi.lm_config_default()
    ver, _ = capi.loop_verify(ws, cfg, L["q"], DIVISOR, L["cands"], L["vcands"], L["pre"], L["raw"], L["ikp"], MG_WEIGHT)
    B, H, W = L["B"], 32, 40
    vy, vx = np.divmod(np.arange(H * W), W)
    homo = cu(np.stack([(vx - cam.cx) / cam.fx, (vy - cam.cy) / cam.fy, np.ones(H * W)], 1))
    loc = cu(np.arange(H * W), np.int64)
    scands = [dict(id=100 + 3 * b, valid_loc1d=loc, valid_homo=homo, dpt_scale=1.0 + 0.5 * b, tracker_ref_scale=float(ver[b].scale) or 1.0)
              for b in range(B)]
    bias = L["cands"][0]["dpt_map"].reshape(H, W)                     # any positive map of the query's size
    mask = cu(np.ones((H, W)))
    acfg = dict(min_area_ratio=0.0, min_inlier_ratio=0.0, base_metric=0.0, base_desc_ratio=0.0, redundant_range=5, dpt_eps=1e-4)
    infos, kept = capi.loop_accept(ws, accept_cfg(capi, acfg), bias, mask, cam, L["cands"], scands, L["pre"], ver)
    cands = [dict(tracked=ver[b].tracked, status=ver[b].status, area_ratio=ver[b].area_ratio, inlier_ratio=ver[b].inlier_ratio,
                  area_inlier_ratio=ver[b].area_inlier_ratio, desc=L["pre"][b].desc_match_inlier_ratio, pose12=np.array(ver[b].pose12[:], F),
                  id=scands[b]["id"], dpt_scale=scands[b]["dpt_scale"], tracker_ref_scale=scands[b]["tracker_ref_scale"]) for b in range(B)]
    acc, want_kept = check_against_the_restatement(capi, ws, acfg, cands, L["cands"], scands, bias, mask, cam, infos, kept)
    assert [bool(ver[b].tracked) for b in range(B)] == [True, False, False, True]
    assert not acc[1] and not acc[2] and len(kept) == sum(acc) > 0    # ids 9 apart: nothing is redundant
