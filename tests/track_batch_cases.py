"""The mixed batches of the batched tracker's tests (tests/test_track_lm_batch.py on the CPU oracle, tests/test_gpu_track_batch.py
on the device): five problems on the scene tests/edge_scenes.LM_SCENE whose LM trajectories differ in length and in branch, so
that the rounds of a batch mix linearize and error requests and problems drop out one after the other.  No GPU, no engine
library.

A batch has ONE configuration and one term composition (sage_track_frame_batch demands the latter), so the
cases are spread over three compositions, each with five starts, and the iteration cap is a second configuration of the same batch:

  composition                      no_overlap_error   starts (multiples of the LM_START offset, rotation and translation)
  dof 6 photo + reprojection       off                1 | converged | 8 | far | -3
  dof 7 photo only                 9.9 * sum(w)       1 | converged | 1.5 | far | -1      ("far" leaves with SAGE_E_NO_OVERLAP)
  dof 7 photo + match geometry     off                1 | converged | 8 | far | (-2, 2)

"converged" is the true pose at the true scale (one iteration, rejected at max_damp); "far" is the 50-unit translation of
test_track_frame_no_overlap_exit; 8 and 1.5 are far enough that steps are rejected and the damping climbs to max_damp.
Measured on the fp32 oracle, iterations per start: 4 1 6 3 8 | 5 1 8 0 5 | 4 1 7 3 6 (tests/test_track_lm_batch.py asserts
what the batch tests rely on: at least three different counts and a rejected step)."""
import numpy as np

from tests import edge_scenes as es

COMPOSITIONS = [(6, True, True), (7, True, False), (7, True, True)]
COMPOSITION_IDS = ["dof6_photo+reproj", "dof7_photo", "dof7_photo+matchgeom"]
_STARTS = {(6, True, True): (1, "converged", 8, "far", -3),
           (7, True, False): (1, "converged", 1.5, "far", -1),
           (7, True, True): (1, "converged", 8, "far", (-2, 2))}
CAP = 2                                     # max_num_iters of the capped configuration: cuts the first start's run


def configure(capi, scene, dof, use_photo, use_kp, capped=False):
    cfg = capi.lm_config_default()
    if dof == 7 and not use_kp:             # TrackFrame without the match-geometry term (camera_tracker.cpp:1515)
        cfg.no_overlap_error = 9.9 * float(np.sum(scene.w.photo_weights))
    if capped:
        cfg.max_num_iters = CAP
    return cfg


def starts(scene, dof, use_photo, use_kp):
    """-> [(pose12, scale)] of the composition's five problems on a HostScene"""
    rot, trans = np.array(es.LM_START["rot"]), np.array(es.LM_START["trans"])
    low = np.float32(float(scene.s_true) * (0.96 if dof == 7 else 1.0))
    out = []
    for k in _STARTS[(dof, use_photo, use_kp)]:
        if k == "converged":
            out.append((scene.start_pose((0, 0, 0), (0, 0, 0)), np.float32(scene.s_true)))
        elif k == "far":
            p = scene.start_pose().copy()
            p[9:] += np.array([50.0, 0, 0], np.float32)
            out.append((p, low))
        else:
            kr, kt = k if isinstance(k, tuple) else (k, k)
            out.append((scene.start_pose(tuple(kr * rot), tuple(kt * trans)), low))
    return out


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def assert_row_equals_single(row, single, what=""):
    """row / single: (status, pose12, scale, error, iters, trace) with float32 values; equal as BYTES"""
    st_b, p_b, s_b, e_b, it_b, tr_b = row
    st_s, p_s, s_s, e_s, it_s, tr_s = single
    assert st_b == st_s and it_b == it_s, what
    assert same_bytes(np.float32(p_b), np.float32(p_s)), what
    assert same_bytes(np.float32(s_b), np.float32(s_s)) and same_bytes(np.float32(e_b), np.float32(e_s)), what
    assert len(tr_b) == len(tr_s), what
    for g, w in zip(tr_b, tr_s):
        for k in ("damp", "error", "candidate_error"):
            assert same_bytes(np.float32(g[k]), np.float32(w[k])), (what, k)
        assert g["accepted"] == w["accepted"] and g["relinearized"] == w["relinearized"], what
