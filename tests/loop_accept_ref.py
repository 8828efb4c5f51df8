"""A pure-Python / numpy restatement of sage_loop_accept's host rules, written from include/sage_ba.h: the accept test, the
pose hand-over, the sort and the redundancy filter (loop_detector.cpp:173-229).  All arithmetic in np.float32, one rounding
per operation.

A candidate is a dict: tracked, status, area_ratio, inlier_ratio, area_inlier_ratio (sage_loop_verify's), desc
(pre.desc_match_inlier_ratio), pose12 [12], id, dpt_scale, tracker_ref_scale.  cfg is a dict: min_area_ratio,
min_inlier_ratio, base_metric, base_desc_ratio, redundant_range."""
import numpy as np

f32 = np.float32


def accepted(cfg, c) -> bool:
    """(a NaN fails every comparison, as in C++)"""
    if not c["tracked"] or c["status"] != 0:
        return False
    if not (f32(c["area_ratio"]) >= f32(cfg["min_area_ratio"])) or not (f32(c["inlier_ratio"]) >= f32(cfg["min_inlier_ratio"])):
        return False
    return bool(f32(c["area_inlier_ratio"]) >= f32(cfg["base_metric"]) and f32(c["desc"]) >= f32(cfg["base_desc_ratio"]))


def pose(pose12, dpt_scale, tracker_ref_scale):
    """-> (R_cur_ref [3,3], t_cur_ref [3]) float32: the inverse of (R, t), the translation times dpt_scale, then divided by
    tracker_ref_scale"""
    p = np.asarray(pose12, f32).reshape(12)
    R, t = p[:9].reshape(3, 3), p[9:]
    Rt = np.ascontiguousarray(R.T)
    out = np.zeros(3, f32)
    for i in range(3):
        a, b, c = f32(-R[0, i]) * t[0], f32(-R[1, i]) * t[1], f32(-R[2, i]) * t[2]
        ti = f32(f32(a + b) + c)
        out[i] = f32(f32(ti * f32(dpt_scale)) / f32(tracker_ref_scale))
    return Rt, out


def filter_kept(cfg, cands):
    """-> (accepted flags [B], kept_order: the kept candidates' indices by descending desc, ties in candidate order, a
    candidate dropped when its id is within redundant_range of one kept before it)"""
    acc = [accepted(cfg, c) for c in cands]
    order = sorted([b for b in range(len(cands)) if acc[b]], key=lambda b: -float(f32(cands[b]["desc"])))   # (sorted is stable)
    kept = []
    for b in order:
        if all(not (abs(int(cands[k]["id"]) - int(cands[b]["id"])) < int(cfg["redundant_range"])) for k in kept):
            kept.append(b)
    return acc, kept
