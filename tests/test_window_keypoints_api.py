"""Matched-keypoint terms of the window engine (sage_window_add_keypoint_term), the parts that need no GPU: header,
exports, ctypes mirror, argument validation before any device call, and the synthetic match generators."""
import ctypes as C
import os
import re

import numpy as np

from sage_slam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sage_window_add_keypoint_term", "sage_window_num_keypoint_terms", "sage_window_get_keypoint_term")


def test_header_declares_and_library_exports_the_keypoint_term_api():
    hdr = open(os.path.join(ROOT, "include", "sage_ba.h")).read()
    L = capi.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in capi.SYMBOLS
    body = re.search(r"typedef struct SageKeypointTerm\s*\{(.*?)\}\s*SageKeypointTerm;", hdr, re.S)
    assert body, "struct SageKeypointTerm missing"
    # the ctypes mirror lists the header's fields in the header's order
    fields = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
    assert fields == [f[0] for f in capi.SageKeypointTerm._fields_]
    assert re.search(r"SAGE_KP_REPROJECTION\s*=\s*0\s*,\s*SAGE_KP_MATCH_GEOMETRY\s*=\s*1", hdr)
    assert (capi.SAGE_KP_REPROJECTION, capi.SAGE_KP_MATCH_GEOMETRY) == (0, 1)
    assert "which` 4" in hdr or "4 keypoint-term linearize" in hdr      # sage_window_get_kernel_time documents 4 / 5


def test_bad_calls_answer_invalid_without_a_device():
    """No window exists without a device, so these are the calls a host without one can make: every one is answered from
    the argument checks (tests/test_gpu_window_keypoints.py repeats bad edge / N / kind on a live window)."""
    L = capi.lib()
    INVALID = -1
    assert L.sage_window_add_keypoint_term(None, None) == INVALID
    assert L.sage_window_num_keypoint_terms(None) == 0
    assert L.sage_window_get_keypoint_term(None, 0, None, None, None, None) == INVALID
    for kind, edge, n in ((0, 0, 1), (0, -1, 8), (0, 0, 0), (7, 0, 8)):
        t = capi.SageKeypointTerm()
        t.kind, t.edge, t.N = kind, edge, n
        t.loss_param, t.weight = 1.0, 1.0
        assert L.sage_window_add_keypoint_term(None, C.byref(t)) == INVALID


def test_match_generators_are_deterministic_and_in_image():
    w = synth.make_window(K=4, H=48, W=64, FS=16, CS=16, L=3, n_samples=600, seed=3)
    for make, keys in ((synth.make_reprojection_matches, ("loc0", "homo0", "matched_2d")),
                       (synth.make_match_geometry_matches, ("loc0", "homo0", "loc1", "homo1"))):
        a, b, c = make(w, 0, 1, 96, 11), make(w, 0, 1, 96, 11), make(w, 0, 1, 96, 12)
        assert sorted(k for k in a if k != "kind") == sorted(keys)
        assert all(np.array_equal(a[k], b[k]) for k in keys)
        assert any(not np.array_equal(a[k], c[k]) for k in keys)
        assert a["loc0"].dtype == np.int32 and a["loc0"].shape == (96,) and a["homo0"].shape == (96, 3)
        assert a["loc0"].min() >= 0 and a["loc0"].max() < w.H * w.W
        assert np.isin(a["loc0"], w.keyframes[0].loc1d).all()                   # drawn from keyframe 0's samples
    r = synth.make_reprojection_matches(w, 0, 1, 96, 11, noise_px=0.0, outlier_share=0.0)
    m = synth.make_match_geometry_matches(w, 0, 1, 96, 11, noise_px=0.0, outlier_share=0.0)
    assert r["matched_2d"].dtype == np.float32 and r["matched_2d"].shape == (96, 2)
    assert m["loc1"].dtype == np.int32 and m["loc1"].min() >= 0 and m["loc1"].max() < w.H * w.W
    # the match is the rounded pixel of the projection, the ray is that pixel's
    x, y = m["loc1"] % w.W, m["loc1"] // w.W
    inside = (r["matched_2d"][:, 0] > 0) & (r["matched_2d"][:, 0] < w.W - 1) & (r["matched_2d"][:, 1] > 0) & \
        (r["matched_2d"][:, 1] < w.H - 1)
    assert inside.sum() > 48
    assert np.abs(x - r["matched_2d"][:, 0])[inside].max() <= 0.5 + 1e-4
    assert np.abs(y - r["matched_2d"][:, 1])[inside].max() <= 0.5 + 1e-4
    cam = w.cams[0]
    assert np.allclose(m["homo1"][:, 0], (x - cam.cx) / cam.fx, atol=1e-6) and np.all(m["homo1"][:, 2] == 1)
    # without noise the true variables reproject onto the match: the same projection through the oracle's conventions
    a0, a1 = w.keyframes[0], w.keyframes[1]
    d = a0.scale_true * (a0.bias[r["loc0"]] + a0.basis[r["loc0"]] @ a0.code_true)
    R10, t10 = synth.relative_pose(a0.R_true, a0.t_true, a1.R_true, a1.t_true)
    X = (R10 @ (d[:, None] * r["homo0"]).T).T + t10
    px = np.stack([X[:, 0] / X[:, 2] * cam.fx + cam.cx, X[:, 1] / X[:, 2] * cam.fy + cam.cy], 1)
    assert np.abs(px - r["matched_2d"]).max() < 1e-2
