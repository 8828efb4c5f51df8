"""Preconditions of the edge-shape GPU suites (tests/test_gpu_tracker_shapes.py, tests/test_gpu_producer_shapes.py) on the
scenes of tests/edge_scenes.py, checked on the CPU against the fp32 oracle alone: conditions on the INPUTS, so that a
passing GPU test means something."""
import numpy as np
import pytest

from tests import edge_scenes as es
from tests.helpers import rel


@pytest.mark.parametrize("case", es.TRACKER_CASES, ids=es.tracker_case_id)
def test_tracker_case_has_mixed_validity_and_a_live_heavy_tail(orc, case):
    s = es.tracker_scene(**case)
    assert s.N == (case["N"] or 40 * 52)
    tail = es.tail_samples(case)
    for dof in (6, 7):
        o = es.oracle_jac(orc, s, dof)
        # mixed validity: some samples count, some do not (one sample cannot be both: N = 1 has its one inlier)
        assert 0 < o["num_inliers"] <= s.N and (o["num_inliers"] < s.N or s.N == 1)
        # the last sample is an inlier
        without_last = es.oracle_jac(orc, s, dof, n=s.N - 1) if s.N > 1 else dict(num_inliers=0, AtA=np.zeros((dof, dof)))
        assert o["num_inliers"] - without_last["num_inliers"] == 1
        # ... and the tail carries weight: without it AtA is 100 bars away, a lost tail lane or tile cannot pass
        bar = es.tracker_bars(orc, s, dof)[3]["AtA"]
        without_tail = without_last if tail == 1 else es.oracle_jac(orc, s, dof, n=s.N - tail)
        assert rel(without_tail["AtA"], o["AtA"]) >= 100 * bar
        assert rel(without_last["AtA"], o["AtA"]) >= 2 * bar       # (the dense case: see edge_scenes.tail_samples)


def test_negative_depth_pattern_spares_the_last_sample():
    for n in (1, 2, 7, 8, 63, 64, 65, 257, 2080):
        idx = es.negative_depth_indices(n)
        assert n - 1 not in idx and (n < 8 or len(idx) >= n // 7)
    assert 0 in es.negative_depth_indices(63) and 63 in es.negative_depth_indices(65)


@pytest.mark.parametrize("dof", [6, 7])
def test_zero_inlier_scene_has_no_inlier(orc, dof):
    s = es.tracker_scene(**es.ZERO_INLIER_CASE, far=True)
    o = es.oracle_jac(orc, s, dof)
    assert o["num_inliers"] == 0 and not o["AtA"].any() and not o["Atb"].any()
    assert o["error"] == 10.0 * float(s.weights.sum())
    assert es.oracle_err(orc, s) == (10.0 * float(s.weights.sum()), 0.0)


@pytest.mark.parametrize("dof,use_photo,use_kp", es.LM_COMPOSITIONS)
def test_lm_run_has_no_decision_near_a_tie(orc, dof, use_photo, use_kp):
    """the oracle's own LM run at the second shape: every accept / reject decision is 1e-2 of the error away from a tie,
    over at least three iterations with a step"""
    from sage_slam_amd import capi
    from tests.tracker_scene import HostScene
    scene = HostScene(orc, **es.LM_SCENE)
    assert scene.a.homo.shape == (257, 3) and scene.w.FS == 32 and scene.w.L == 2 and scene.NK == 65
    lin, err, decisions = es.recording_callbacks(*scene.oracle_callbacks(dof, use_photo, use_kp))
    s0 = float(scene.s_true) * (0.96 if dof == 7 else 1.0)
    _, _, _, iters, trace = capi.track_lm(capi.lm_config_default(), dof, lin, err, scene.start_pose(**es.LM_START), s0)
    assert es.decided_iterations(decisions, iters) == iters
    assert len(trace) >= es.LM_MIN_ITERS and all(t["accepted"] for t in trace[:es.LM_MIN_ITERS])
    # the recorder saw what the policy did: one decision per traced iteration here, the same errors
    assert [(e, c) for _, e, c in decisions] == [(t["error"], t["candidate_error"]) for t in trace]


def test_tracker_scene_defaults_are_the_golden_scene(orc):
    """tests/tracker_scene.HostScene grew keyword arguments: its defaults are still the BASELINE config-1 scene"""
    from tests.tracker_scene import HostScene
    s = HostScene(orc)
    assert (s.w.H, s.w.W, s.w.FS, s.w.L, s.a.homo.shape[0], s.NK) == (64, 80, 16, 4, 3072, 160)


@pytest.mark.parametrize("case", es.PYRAMID_CASES, ids=lambda c: f"{c['H']}x{c['W']}")
def test_holey_mask_has_dead_and_half_dead_texels(case):
    H, W = case["H"], case["W"]
    m = es.pyramid_mask("holey", H, W)
    assert 0.6 < m.mean() < 0.85
    levels = es.mask_levels(m, 3)
    assert [lv.shape for lv in levels] == [(H, W), (H // 2, W // 2), (H // 2 // 2, W // 2 // 2)]
    assert np.array_equal(levels[1], m[::2, ::2][:H // 2, :W // 2])
    for l in (0, 1):                                  # the taps of the level-1 and of the level-2 texels
        live, have = es.live_taps(levels[l])
        assert live.shape == levels[l + 1].shape and have.max() == 9 and have.min() == 4
        assert (live == 0).any(), f"level {l + 1}: no texel without a live tap"
        assert ((live > 0) & (live < have)).any(), f"level {l + 1}: no texel with some dead taps"
    # the other kinds: what their names say
    assert es.pyramid_mask("ones", H, W).all() and not es.pyramid_mask("zeros", H, W).any()
    syn = es.pyramid_mask("synthetic", H, W)
    assert syn[2:-2, 2:-2].all() and syn.sum() == (H - 4) * (W - 4)


def test_live_taps_against_a_direct_count():
    m = es.pyramid_mask("holey", 10, 14, seed=3)
    live, have = es.live_taps(m)
    for y in range(5):
        for x in range(7):
            taps = [(2 * y + dy, 2 * x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            inside = [(a, b) for a, b in taps if 0 <= a < 10 and 0 <= b < 14]
            assert have[y, x] == len(inside) and live[y, x] == sum(m[a, b] != 0 for a, b in inside)


@pytest.mark.parametrize("H,W", es.LOCATION_SHAPES, ids=lambda v: str(v))
def test_location_masks_cover_the_chunk_tail(orc, H, W):
    HW = H * W
    first_of_last = (HW - 1) // es.CHUNK * es.CHUNK
    cam = es.location_camera(H, W)
    n = {k: len(orc.valid_locations(es.location_mask(k, H, W), cam)[0]) for k in es.LOCATION_MASKS}
    assert n["zeros"] == 0 and n["ones"] == HW and n["last_pixel"] == 1 and n["last_chunk"] == HW - first_of_last
    assert 0 < n["random"] < HW and 0 < n["threshold"] < HW
    loc, _ = orc.valid_locations(es.location_mask("last_chunk", H, W), cam)
    assert loc[0] == first_of_last and loc[-1] == HW - 1
    thr = es.location_mask("threshold", H, W).reshape(-1)
    tloc, _ = orc.valid_locations(thr.reshape(H, W), cam)
    assert (thr == 0.5).sum() >= HW // 5 and not np.isin(np.nonzero(thr == 0.5)[0], tloc).any()     # 0.5 is not > 0.5
    above = np.nonzero(thr == np.nextafter(np.float32(0.5), np.float32(1)))[0]
    assert len(above) >= HW // 5 and np.isin(above, tloc).all() and tloc[-1] == HW - 1
    # the shapes are what they are for: below one chunk, one chunk, one chunk + 1, a partial fourth chunk
    assert [h * w - es.CHUNK * ((h * w) // es.CHUNK) for h, w in es.LOCATION_SHAPES] == [768, 0, 1, 28]
