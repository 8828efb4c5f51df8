"""ctypes binding of the C ABI (``include/sage_ba.h``) + thin torch plumbing.

PyTorch is used only for device memory (``torch.Tensor.data_ptr()``), streams and
``torch.distributed``; every compute entry point goes through ``libsage_ba.so``.
There is no CPU fallback: if the library is missing or no HIP device is present the
calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsage_ba.so")
SAGE_MAX_LEVELS = 8


class SageError(RuntimeError):
    def __init__(self, code: int, where: str):
        self.code = code
        msg = lib().sage_error_string(code).decode() if _lib is not None else "?"
        super().__init__(f"{where}: {msg} (code {code})")


class SageCamera(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "w", "h")]


class SagePyramid(C.Structure):
    _fields_ = [("levels", C.c_int32), ("P", C.c_int32), ("level_offsets", C.c_int32 * SAGE_MAX_LEVELS),
                ("cam", SageCamera * SAGE_MAX_LEVELS)]


class SageLmConfig(C.Structure):
    _fields_ = [("max_num_iters", C.c_int), ("min_grad_thresh", C.c_float), ("min_param_inc_thresh", C.c_float),
                ("init_damp", C.c_float), ("min_damp", C.c_float), ("max_damp", C.c_float),
                ("damp_dec_factor", C.c_float), ("damp_inc_factor", C.c_float),
                ("jac_update_err_inc_threshold", C.c_float), ("max_inner_evals", C.c_int),
                ("no_overlap_error", C.c_float), ("linearize_at_candidate", C.c_int)]


class SageLmTraceEntry(C.Structure):
    _fields_ = [("damp", C.c_float), ("error", C.c_float), ("candidate_error", C.c_float),
                ("accepted", C.c_int), ("relinearized", C.c_int)]


class SageTrackProblem(C.Structure):
    _fields_ = [("ws", C.c_void_p), ("use_photo", C.c_int32), ("mask1_dev", C.c_void_p), ("dpts0_dev", C.c_void_p),
                ("homo_dev", C.c_void_p), ("feat0s_dev", C.c_void_p), ("feat1_dev", C.c_void_p),
                ("grad1_dev", C.c_void_p), ("weights_dev", C.c_void_p), ("pyr", SagePyramid), ("eps", C.c_float),
                ("N", C.c_int32), ("FS", C.c_int32), ("use_keypoints", C.c_int32), ("NK", C.c_int32),
                ("kp_dpts0_dev", C.c_void_p), ("kp_homo0_dev", C.c_void_p), ("kp_matched_2d_dev", C.c_void_p),
                ("kp_matched_dpts1_dev", C.c_void_p), ("kp_matched_homo1_dev", C.c_void_p),
                ("kp_loss_param", C.c_float), ("kp_weight", C.c_float)]


class SageKeyframeView(C.Structure):
    _fields_ = [("feat_pyr", C.c_void_p), ("grad_pyr", C.c_void_p), ("bias", C.c_void_p), ("basis", C.c_void_p),
                ("loc1d", C.c_void_p), ("homo", C.c_void_p), ("N", C.c_int32)]


class SageWindowConfig(C.Structure):
    _fields_ = [("pyr", SagePyramid), ("FS", C.c_int32), ("CS", C.c_int32), ("mask_dev", C.c_void_p),
                ("photo_weights", C.c_float * SAGE_MAX_LEVELS), ("geo_weight", C.c_float),
                ("geo_loss_param", C.c_float), ("eps", C.c_float), ("code_prior_weight", C.c_float),
                ("scale_prior_weight", C.c_float), ("pose_prior_weight", C.c_float),
                ("use_photo", C.c_int32), ("use_geo", C.c_int32)]


SAGE_KP_REPROJECTION, SAGE_KP_MATCH_GEOMETRY, SAGE_KP_LOOP_MG = 0, 1, 2
SAGE_HOLD_POSE, SAGE_HOLD_CODE, SAGE_HOLD_SCALE = 1, 2, 4
KP_KINDS = {"reprojection": SAGE_KP_REPROJECTION, "match_geometry": SAGE_KP_MATCH_GEOMETRY, "loop_mg": SAGE_KP_LOOP_MG}


class SageKeypointTerm(C.Structure):
    _fields_ = [("kind", C.c_int32), ("edge", C.c_int32), ("N", C.c_int32), ("loc1d_0", C.c_void_p), ("homo0", C.c_void_p),
                ("matched_2d", C.c_void_p), ("matched_loc1d_1", C.c_void_p), ("matched_homo1", C.c_void_p),
                ("loss_param", C.c_float), ("weight", C.c_float), ("loss", C.c_int32), ("unscaled_dpts0", C.c_void_p),
                ("matched_unscaled_dpts1", C.c_void_p)]


def kp_term_dim(kind, CS: int) -> int:
    """system size D of a window keypoint term by kind (name or SAGE_KP_*)"""
    kind = KP_KINDS.get(kind, kind)
    return {SAGE_KP_REPROJECTION: 13 + CS, SAGE_KP_MATCH_GEOMETRY: 14 + 2 * CS, SAGE_KP_LOOP_MG: 14}[kind]


SAGE_GRAPH_REL_POSE_SCALE, SAGE_GRAPH_REL_POSE, SAGE_GRAPH_SCALE_PRIOR = 0, 1, 2
GRAPH_KINDS = {"rel_pose_scale": SAGE_GRAPH_REL_POSE_SCALE, "rel_pose": SAGE_GRAPH_REL_POSE, "scale_prior": SAGE_GRAPH_SCALE_PRIOR}
GRAPH_TERM_DIM = 14                      # [pose0 pose1 scale0 scale1] for every kind
GRAPH_KIND_ROWS = {SAGE_GRAPH_REL_POSE_SCALE: 7, SAGE_GRAPH_REL_POSE: 6, SAGE_GRAPH_SCALE_PRIOR: 1}


class SageGraphTerm(C.Structure):
    _fields_ = [("kind", C.c_int32), ("edge", C.c_int32), ("kf", C.c_int32), ("target_pose10", C.c_float * 12),
                ("target_scale0", C.c_float), ("target_scale1", C.c_float), ("weight", C.c_float), ("rot_weight", C.c_float),
                ("scale_weight", C.c_float)]


def graph_term_struct(t) -> SageGraphTerm:
    """dict -> ``SageGraphTerm``: kind (a GRAPH_KINDS name or SAGE_GRAPH_*), edge or kf, target_pose10 [12] (R row-major, t),
    target_scale0 / target_scale1, weight, rot_weight, scale_weight; what a kind does not use may be left out."""
    gt = SageGraphTerm()
    gt.kind = int(GRAPH_KINDS.get(t["kind"], t["kind"]))
    gt.edge, gt.kf = int(t.get("edge", 0)), int(t.get("kf", 0))
    tp = np.asarray(t.get("target_pose10", [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), np.float32).reshape(12)
    for i in range(12):
        gt.target_pose10[i] = float(tp[i])
    gt.target_scale0, gt.target_scale1 = float(t.get("target_scale0", 1.0)), float(t.get("target_scale1", 1.0))
    gt.weight, gt.rot_weight, gt.scale_weight = float(t["weight"]), float(t.get("rot_weight", 1.0)), float(t.get("scale_weight", 1.0))
    return gt


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)


class SageLmState(C.Structure):
    _fields_ = [("damp", C.c_double), ("error", C.c_double), ("candidate_error", C.c_double),
                ("accepted", C.c_int), ("iters", C.c_int)]


SAGE_DOGLEG_SEARCH_EACH_ITERATION, SAGE_DOGLEG_SEARCH_REDUCE_ONLY, SAGE_DOGLEG_ONE_STEP_PER_ITERATION = 0, 1, 2
DOGLEG_DOTS = ("gg", "gn", "nn", "gAg", "gAn", "nAn")     # the order of every dots [6]


class SageDoglegConfig(C.Structure):
    _fields_ = [("init_delta", C.c_double), ("min_delta", C.c_double), ("mode", C.c_int)]


class SageDoglegState(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("delta", "error", "candidate_error", "rho", "step_norm", "sd_norm", "gn_norm", "a", "b")] + \
               [("dots", C.c_double * 6)] + \
               [(n, C.c_int) for n in ("region", "accepted", "evals", "solves", "iters")]


DOGLEG_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_double))


def dogleg_config_default() -> SageDoglegConfig:
    cfg = SageDoglegConfig()
    lib().sage_dogleg_config_default(C.byref(cfg))
    return cfg


def dogleg_point(delta, gg, gn, nn, gAg):
    """``sage_dogleg_point`` -> (status code, a, b, region): the dogleg point for radius ``delta`` is a g + b n"""
    f = lib().sage_dogleg_point
    f.argtypes = [C.c_double] * 5 + [C.c_void_p] * 3
    a, b, region = C.c_double(), C.c_double(), C.c_int()
    rc = int(f(delta, gg, gn, nn, gAg, C.addressof(a), C.addressof(b), C.addressof(region)))
    return rc, a.value, b.value, region.value


def dogleg_iterate(cfg: SageDoglegConfig, dots, f_error, fn, state: SageDoglegState) -> int:
    """``sage_dogleg_iterate`` around the Python callable ``fn(a, b) -> error`` (an exception ends the iteration with
    SAGE_E_STATE) -> status code; ``state`` is updated in place."""
    d = np.ascontiguousarray(dots, np.float64)
    assert d.size == 6

    def tramp(_ctx, a, b, out):
        try:
            out[0] = float(fn(a, b))
            return 0
        except Exception:                          # never unwind through the C frames
            import traceback
            traceback.print_exc()
            return -4

    f = lib().sage_dogleg_iterate
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, DOGLEG_EVAL_FN, C.c_void_p, C.c_void_p]
    return int(f(C.addressof(cfg), d.ctypes.data, float(f_error), DOGLEG_EVAL_FN(tramp), None, C.addressof(state)))


def dogleg_incidence(K: int, links):
    """``sage_dogleg_incidence`` -> (status code, offsets [K + 1], entries [K + 2 nlinks, 2] of (block, transposed))"""
    lk = np.ascontiguousarray(np.asarray(links, np.int32).reshape(-1, 2))
    off = np.zeros(max(K, 0) + 1, np.int32)
    ent = np.zeros((max(K, 0) + 2 * len(lk), 2), np.int32)
    f = lib().sage_dogleg_incidence
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = int(f(int(K), len(lk), lk.ctypes.data if len(lk) else None, off.ctypes.data, ent.ctypes.data))
    return rc, off, ent


TRACK_LIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float),
                           C.POINTER(C.c_float), C.POINTER(C.c_float))
TRACK_ERR_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_float))

_lib = None

# every symbol include/sage_ba.h declares (checked by tests/test_capi_symbols.py against the header)
SAGE_RELIN_ALL, SAGE_RELIN_STALE = 0, 1


class SageEvalCounts(C.Structure):
    """what the last ``sage_window_linearize`` evaluated (``sage_window_last_evaluation``)"""
    _fields_ = [(n, C.c_int32) for n in ("photo_edges", "geo_edges", "depth_maps", "depth_grads", "photo_items", "geo_items",
                                         "host_entries_pulled")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SageRelinThresholds(C.Structure):
    _fields_ = [("pose", C.c_float * 6), ("code", C.c_float), ("scale", C.c_float)]


def relin_thresholds(pose=1e-3, code=1e-4, scale=1e-3) -> SageRelinThresholds:
    """per-key thresholds (the mapper's: p 1e-3, c 1e-4, s 1e-3); ``pose``: one value or six"""
    t = SageRelinThresholds()
    for i, v in enumerate(np.broadcast_to(np.asarray(pose, np.float32), (6,))):
        t.pose[i] = float(v)
    t.code, t.scale = float(code), float(scale)
    return t


def relin_plan_raw(K, CS, n_links, links_ptr, old_ptrs, new_ptrs, photo_ptr, geo_ptr, map_ptr, n_photo_ptr, n_geo_ptr) -> int:
    """``sage_relin_plan`` on raw pointers (``old_ptrs`` / ``new_ptrs``: pose, code, scale) -> status code"""
    f = lib().sage_relin_plan
    f.argtypes = [C.c_int] * 3 + [C.c_void_p] * 12
    return int(f(int(K), int(CS), int(n_links), links_ptr, *old_ptrs, *new_ptrs, photo_ptr, geo_ptr, map_ptr, n_photo_ptr, n_geo_ptr))


def relin_plan(K: int, CS: int, links, old, new) -> dict:
    """``sage_relin_plan``: ``old`` / ``new`` = (pose [K,12], code [K,CS], scale [K]) -> dict(photo_stale, geo_stale
    [2 * n_links] uint8, map_read [K] uint8, n_photo, n_geo)"""
    lk = np.ascontiguousarray(np.asarray(links, np.int32).reshape(-1, 2))
    o = [_f32(np.asarray(a).reshape(-1)) for a in old]; n = [_f32(np.asarray(a).reshape(-1)) for a in new]
    assert all(a.size == b.size == m for a, b, m in zip(o, n, (K * 12, K * CS, K)))
    ph = np.zeros(2 * len(lk), np.uint8); ge = np.zeros(2 * len(lk), np.uint8); mr = np.zeros(K, np.uint8)
    n_p, n_g = C.c_int32(), C.c_int32()
    _chk(relin_plan_raw(K, CS, len(lk), lk.ctypes.data, [a.ctypes.data for a in o], [a.ctypes.data for a in n], ph.ctypes.data,
                        ge.ctypes.data, mr.ctypes.data, C.addressof(n_p), C.addressof(n_g)), "sage_relin_plan")
    return dict(photo_stale=ph, geo_stale=ge, map_read=mr, n_photo=n_p.value, n_geo=n_g.value)


def relin_marks_raw(delta_ptr, K, CS, t_ptr, marks_ptr, n_marked_ptr) -> int:
    f = lib().sage_relin_marks
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(delta_ptr, int(K), int(CS), t_ptr, marks_ptr, n_marked_ptr))


def relin_marks(delta, K: int, CS: int, t: SageRelinThresholds):
    """``sage_relin_marks``: delta [K, 7 + CS] -> (marks [K] int32 of SAGE_HOLD_* bits, groups marked)"""
    d = np.ascontiguousarray(delta, np.float64).reshape(-1)
    assert d.size == K * (7 + CS)
    marks = np.zeros(K, np.int32); n = C.c_int32()
    _chk(relin_marks_raw(d.ctypes.data, K, CS, C.addressof(t), marks.ctypes.data, C.addressof(n)), "sage_relin_marks")
    return marks, n.value


SYMBOLS = [
    "sage_camera_pyramid", "sage_version", "sage_error_string", "sage_workspace_create", "sage_workspace_destroy",
    "sage_photometric_jac_error_calculate", "sage_photometric_error_calculate",
    "sage_tracker_photo_jac_error_calculate", "sage_tracker_photo_error_calculate",
    "sage_geometric_jac_error_calculate", "sage_geometric_error_calculate", "sage_depth_and_grad",
    "sage_gaussian_pyramid_with_grad", "sage_se3_exp", "sage_pose_retract", "sage_nearest_psd", "sage_nearest_psd_reference", "sage_factor_block_count", "sage_factor_hessian_blocks",
    "sage_damped_solve_qr_f32", "sage_block_solve", "sage_solve_lookahead_count", "sage_lm_config_default", "sage_track_lm", "sage_track_lm_batch", "sage_track_frame", "sage_track_frame_batch", "sage_track_overlap", "sage_track_overlap_batch", "sage_track_overlap_batch_plan", "sage_track_overlap_batch_launches", "sage_convex_hull_area", "sage_depth_scale_ratio", "sage_median_f32",
    "sage_depth_scale_ratio_batch", "sage_median_f32_batch", "sage_depth_scale_ratio_batch_plan", "sage_depth_scale_ratio_batch_launches",
    "sage_vocabulary_create", "sage_vocabulary_destroy", "sage_vocabulary_num_nodes", "sage_vocabulary_num_words", "sage_vocabulary_channels", "sage_vocabulary_depth", "sage_vocabulary_max_fanout", "sage_vocabulary_staged_nodes",
    "sage_vocabulary_build_config_default", "sage_vocabulary_build", "sage_vocabulary_build_desc", "sage_vocabulary_build_docs_with_word", "sage_vocabulary_build_node_of_point", "sage_vocabulary_build_stats", "sage_vocabulary_build_plan", "sage_vocabulary_build_draw", "sage_vocabulary_build_destroy",
    "sage_bow_transform", "sage_bow_score", "sage_bow_db_create", "sage_bow_db_destroy", "sage_bow_db_add", "sage_bow_db_size", "sage_bow_db_query",
    "sage_window_create", "sage_window_destroy", "sage_window_add_keyframe", "sage_window_add_link", "sage_window_add_keypoint_link", "sage_window_hold", "sage_window_set_link_geo_loss",
    "sage_window_set_shard", "sage_window_finalize", "sage_window_num_keyframes", "sage_window_num_links",
    "sage_window_block_size", "sage_window_solver_block_size", "sage_window_packed_count", "sage_window_packed_dev",
    "sage_window_residuals_per_linearize", "sage_window_bytes_per_linearize", "sage_window_linearize",
    "sage_window_error", "sage_window_tune_runs", "sage_window_set_runs", "sage_window_error_dev", "sage_window_solve", "sage_window_total_error",
    "sage_window_accept", "sage_window_reset", "sage_window_get_keyframe", "sage_window_set_keyframe", "sage_window_get_delta",
    "sage_window_get_edge", "sage_window_add_keypoint_term", "sage_window_num_keypoint_terms", "sage_window_get_keypoint_term", "sage_window_add_graph_term", "sage_window_num_graph_terms", "sage_window_get_graph_term", "sage_window_prepass", "sage_window_factor", "sage_window_factor_error", "sage_term_factor_block_count", "sage_term_factor_blocks", "sage_window_keypoint_factor", "sage_window_keypoint_factor_error", "sage_window_graph_factor", "sage_window_graph_factor_error", "sage_window_prepare_factors", "sage_window_prepare_factors_device", "sage_window_prepare_factors_device_launches", "sage_factor_psd", "sage_factor_psd_batch", "sage_factor_psd_batch_launches", "sage_factor_psd_batch_plan", "sage_jacobi_round_pairs", "sage_factor_cut_blocks", "sage_window_set_profiling", "sage_window_get_kernel_time", "sage_window_get_phase_time", "sage_window_lm_step", "sage_window_lm_run", "sage_window_lm_run_timed", "sage_window_sync_variables", "sage_window_set_allreduce", "sage_shard_plan_create", "sage_shard_plan_create_domains", "sage_block_solve_domains", "sage_shard_plan_destroy", "sage_shard_sep_count", "sage_shard_num_separators", "sage_shard_num_interior", "sage_shard_keyframe_owner", "sage_shard_keyframe_is_local", "sage_shard_eliminate", "sage_shard_solve", "sage_rccl_unique_id", "sage_rccl_comm_create", "sage_rccl_comm_destroy", "sage_rccl_comm_info", "sage_window_use_rccl", "sage_window_emulate_peers", "sage_sort_locations", "sage_bind_thread_to_device", "sage_solver_helper_cpus", "sage_solver_placement_moves", "sage_placement_monitor", "sage_shutdown", "sage_host_threads_running",
    "sage_valid_locations", "sage_shuffle_indices", "sage_sample_locations",
    "sage_reprojection_jac_error_calculate", "sage_reprojection_error_calculate",
    "sage_tracker_reproj_jac_error_calculate", "sage_tracker_reproj_error_calculate",
    "sage_match_geometry_jac_error_calculate", "sage_match_geometry_error_calculate",
    "sage_loop_mg_jac_error_calculate", "sage_loop_mg_error_calculate",
    "sage_tracker_match_geom_jac_error_calculate", "sage_tracker_match_geom_error_calculate", "sage_cycle_match",
    "sage_robust_registration", "sage_tls_estimate", "sage_registration_finish", "sage_match_points",
    "sage_cycle_match_batch", "sage_cycle_match_batch_slices", "sage_loop_precheck", "sage_loop_verify", "sage_loop_accept",
    "sage_robust_registration_batch", "sage_robust_registration_batch_plan", "sage_robust_registration_batch_launches",
    "sage_match_points_batch",
    "sage_workspace_set_registration_finish", "sage_workspace_registration_finish", "sage_registration_finish_batch",
    "sage_registration_finish_plan",
    "sage_dogleg_config_default", "sage_dogleg_point", "sage_dogleg_iterate", "sage_dogleg_incidence",
    "sage_window_dogleg_step", "sage_window_dogleg_run", "sage_window_dogleg_products", "sage_window_dogleg_candidate",
    "sage_window_get_dogleg_vectors",
    "sage_relin_plan", "sage_window_set_relinearization", "sage_window_last_evaluation", "sage_relin_marks",
    "sage_window_relin_marks", "sage_window_accept_marked",
    "sage_keyframe_prepare", "sage_keyframe_prepare_batch", "sage_keyframe_prepare_plan", "sage_keyframe_prepare_launches",
    "sage_keyframe_config_matches", "sage_keyframe_info", "sage_keyframe_get", "sage_keyframe_release",
    "sage_window_add_prepared_keyframe", "sage_window_build_stats",
    "sage_schur_marginal", "sage_marginal_prior_create", "sage_marginal_prior_dims", "sage_marginal_prior_get",
    "sage_marginal_prior_keyframes", "sage_marginal_prior_destroy", "sage_prior_evaluate", "sage_prior_term_plan",
    "sage_window_add_prior_term", "sage_window_num_prior_terms", "sage_window_get_prior_term", "sage_window_marginalize",
    "sage_block_covariance", "sage_covariance_plan", "sage_window_covariance", "sage_window_get_covariance",
    "sage_depth_sigma_batch", "sage_window_depth_sigma", "sage_window_depth_sigma_timing",
    "sage_tsdf_frustum_bounds", "sage_tsdf_plan", "sage_tsdf_create", "sage_tsdf_destroy", "sage_tsdf_reset", "sage_tsdf_get",
    "sage_tsdf_dev", "sage_tsdf_integrate", "sage_tsdf_integrate_batch", "sage_tsdf_integrate_batch_launches",
    "sage_tsdf_view_chunk", "sage_tsdf_last_stats", "sage_window_depth_range", "sage_window_fuse_tsdf",
]


def lib():
    """Load ``libsage_ba.so`` (built in-tree by ``sage_slam_amd.build``); fails loudly when absent."""
    global _lib
    if _lib is None:
        LIB_PATH = os.environ.get("SAGE_BA_LIB", globals()["LIB_PATH"])   # dev: A/B a variant build
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -m sage_slam_amd.build` "
                              "(the HIP engine has no fallback path)")
        # torch first: it bundles its own libamdhip64 (same SONAME); loading it before our library makes both
        # share ONE HIP runtime, so torch device pointers are valid in our launches.  (A C++ host without torch
        # simply binds /opt/rocm's runtime.)
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        L.sage_version.restype = C.c_char_p
        L.sage_error_string.restype = C.c_char_p
        L.sage_window_packed_count.restype = C.c_size_t
        L.sage_shutdown.restype = None
        L.sage_keyframe_release.restype = None
        L.sage_keyframe_release.argtypes = [C.c_void_p]
        L.sage_window_packed_dev.restype = C.c_void_p
        L.sage_window_error_dev.restype = C.c_void_p
        L.sage_window_residuals_per_linearize.restype = C.c_double
        L.sage_window_bytes_per_linearize.restype = C.c_double
        for name in ("sage_window_packed_count", "sage_window_packed_dev", "sage_window_error_dev",
                     "sage_window_residuals_per_linearize", "sage_window_bytes_per_linearize",
                     "sage_window_num_keyframes", "sage_window_num_links", "sage_window_block_size",
                     "sage_window_solver_block_size"):
            getattr(L, name).argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _chk(code: int, where: str):
    if code != 0:
        raise SageError(code, where)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def dptr(t) -> C.c_void_p:
    """device pointer of a torch tensor (must be contiguous)."""
    if t is None:
        return C.c_void_p(0)
    assert t.is_contiguous(), "device buffers handed to the C ABI must be contiguous"
    return C.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------- host helpers
def make_pyramid(cam, levels: int) -> SagePyramid:
    """``CameraPyramid`` (``common/camera_pyramid.h:18-32``) through the C ABI."""
    base = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    out = SagePyramid()
    _chk(lib().sage_camera_pyramid(C.byref(base), levels, C.byref(out)), "sage_camera_pyramid")
    return out


def se3_exp(omega, v):
    omega = _f32(omega); v = _f32(v)
    R = np.zeros(9, np.float32); t = np.zeros(3, np.float32)
    lib().sage_se3_exp(_fp(omega), _fp(v), _fp(R), _fp(t))
    return R.reshape(3, 3), t


def pose_retract(pose12, delta6):
    pose12 = _f32(pose12).reshape(12); delta6 = _f32(delta6)
    out = np.zeros(12, np.float32)
    lib().sage_pose_retract(_fp(pose12), _fp(delta6), _fp(out))
    return out


def nearest_psd(M):
    M = np.ascontiguousarray(M, dtype=np.float64)
    out = np.zeros_like(M)
    _chk(lib().sage_nearest_psd(M.ctypes.data_as(C.POINTER(C.c_double)), M.shape[0],
                                out.ctypes.data_as(C.POINTER(C.c_double))), "sage_nearest_psd")
    return out


def nearest_psd_reference(M):
    M = np.ascontiguousarray(M, np.float64)
    out = np.zeros_like(M)
    _chk(lib().sage_nearest_psd_reference(M.ctypes.data_as(C.POINTER(C.c_double)), M.shape[0],
                                          out.ctypes.data_as(C.POINTER(C.c_double))), "sage_nearest_psd_reference")
    return out


def factor_hessian_blocks(type_: int, CS: int, AtA, Atb, psd_mode: int = 1):
    """sage_factor_hessian_blocks -> (dict {(i, j): G_ij}, [g_i], dims): the HessianFactor blocks of a per-edge system."""
    L = lib()
    A = _f32(AtA); b = _f32(Atb)
    n = L.sage_factor_block_count(type_, CS)
    if n < 0:
        raise SageError(n, "sage_factor_block_count")
    G = np.zeros(n, np.float64); g = np.zeros(b.size, np.float64)
    dims = (C.c_int32 * 6)(); nk = C.c_int32()
    _chk(L.sage_factor_hessian_blocks(type_, CS, _fp(A), _fp(b), psd_mode, G.ctypes.data_as(C.POINTER(C.c_double)),
                                      g.ctypes.data_as(C.POINTER(C.c_double)), dims, C.byref(nk)),
         "sage_factor_hessian_blocks")
    dims = [int(dims[i]) for i in range(nk.value)]
    blocks, gs = _blocks_of(G, g, dims)
    return blocks, gs, dims


TERM_KEYPOINT, TERM_GRAPH = 0, 1                      # SAGE_TERM_*: the family of a window term


def _blocks_of(G, g, dims):
    """the packed upper blocks and g of a factor -> (dict {(i, j): G_ij}, [g_i])"""
    blocks, o = {}, 0
    for i in range(len(dims)):
        for j in range(i, len(dims)):
            blocks[(i, j)] = G[o:o + dims[i] * dims[j]].reshape(dims[i], dims[j]); o += dims[i] * dims[j]
    offs = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    return blocks, [g[offs[i]:offs[i + 1]] for i in range(len(dims))]


def term_factor_block_count(family: int, kind: int, CS: int) -> int:
    """``sage_term_factor_block_count``: doubles of a term factor's packed upper blocks, or the negative status code"""
    return int(lib().sage_term_factor_block_count(int(family), int(kind), int(CS)))


def term_factor_blocks_raw(family, kind, CS, AtA_ptr, Atb_ptr, psd_mode, G_ptr, g_ptr, dims_ptr, nkeys_ptr) -> int:
    """``sage_term_factor_blocks`` with the arguments as given (pointers may be None) -> status code"""
    f = lib().sage_term_factor_blocks
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(family, kind, CS, AtA_ptr, Atb_ptr, psd_mode, G_ptr, g_ptr, dims_ptr, nkeys_ptr))


def term_factor_blocks(family: int, kind: int, CS: int, AtA, Atb, psd_mode: int = 1):
    """``sage_term_factor_blocks`` of a term's system in its group's layout (what ``Window.get_keypoint_term`` /
    ``get_graph_term`` return) -> (dict {(i, j): G_ij}, [g_i], dims): the term's HessianFactor blocks in push order."""
    A = _f32(AtA); b = _f32(Atb)
    n = term_factor_block_count(family, kind, CS)
    if n < 0:
        raise SageError(n, "sage_term_factor_block_count")
    G = np.zeros(n, np.float64); g = np.zeros(b.size, np.float64)
    dims = (C.c_int32 * 6)(); nk = C.c_int32()
    _chk(term_factor_blocks_raw(family, kind, CS, A.ctypes.data, b.ctypes.data, psd_mode, G.ctypes.data, g.ctypes.data,
                                C.addressof(dims), C.addressof(nk)), "sage_term_factor_blocks")
    dims = [int(dims[i]) for i in range(nk.value)]
    blocks, gs = _blocks_of(G, g[:sum(dims)], dims)
    return blocks, gs, dims


PSD_MAX_DIM = 80


class SagePsdStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("sweeps", C.c_int32), ("bump_rounds", C.c_int32), ("min_eig", C.c_double),
                ("off_norm", C.c_double)]


def factor_psd_batch_raw(ws_handle, D, n, AtA_ptr, C_ptr, stats_ptr) -> int:
    """``sage_factor_psd_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_factor_psd_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(ws_handle, int(D), int(n), AtA_ptr, C_ptr, stats_ptr))


def factor_psd_batch(ws: "Workspace", AtA):
    """The Higham projection (``nearest_psd``, psd_mode 1) of every matrix of ``AtA`` -- a contiguous float32 cuda tensor
    [n, D, D] -- on the device through ``sage_factor_psd_batch``: one projection launch and one wait -> (C: float64 cuda
    tensor [n, D, D], a list of n ``SagePsdStats``)."""
    import torch
    assert AtA.dtype == torch.float32 and AtA.dim() == 3 and AtA.shape[1] == AtA.shape[2]
    n, D = int(AtA.shape[0]), int(AtA.shape[1])
    out = torch.empty((n, D, D), dtype=torch.float64, device=AtA.device)
    stats = (SagePsdStats * max(n, 1))()
    # (an empty tensor has no storage: the call checks its pointers before it looks at n)
    ap = dptr(AtA) if n else C.c_void_p(8)
    cp = dptr(out) if n else C.c_void_p(8)
    _chk(factor_psd_batch_raw(ws.h, D, n, ap, cp, C.addressof(stats)), "sage_factor_psd_batch")
    return out, [stats[i] for i in range(n)]


def factor_psd_batch_launches(ws: "Workspace") -> int:
    """kernel launches of the workspace's last ``sage_factor_psd_batch``"""
    f = lib().sage_factor_psd_batch_launches
    f.argtypes = [C.c_void_p]
    return int(f(ws.h if ws is not None else None))


def factor_psd_batch_plan_raw(D, n, lds_ptr, device_ptr, pinned_ptr, launches_ptr) -> int:
    f = lib().sage_factor_psd_batch_plan
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(int(D), int(n), lds_ptr, device_ptr, pinned_ptr, launches_ptr))


def factor_psd_batch_plan(D: int, n: int) -> dict:
    """What a batch of n matrices of D columns takes, through ``sage_factor_psd_batch_plan`` (host only)."""
    lds = C.c_int64(); dev = C.c_int64(); pin = C.c_int64(); launches = C.c_int32()
    _chk(factor_psd_batch_plan_raw(D, n, C.addressof(lds), C.addressof(dev), C.addressof(pin), C.addressof(launches)),
         "sage_factor_psd_batch_plan")
    return dict(lds_bytes=lds.value, device_bytes=dev.value, pinned_bytes=pin.value, launches=launches.value)


def jacobi_round_pairs_raw(D, round_, pairs_ptr) -> int:
    f = lib().sage_jacobi_round_pairs
    f.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return int(f(int(D), int(round_), pairs_ptr))


def jacobi_round_pairs(D: int, round_: int) -> list:
    """The disjoint index pairs round ``round_`` of a Jacobi sweep rotates at once (``sage_jacobi_round_pairs``, host only)
    -> a list of D // 2 tuples (p, q), p < q."""
    pairs = (C.c_int32 * max(2 * (int(D) // 2), 2))()
    n = jacobi_round_pairs_raw(D, round_, C.addressof(pairs))
    if n < 0:
        raise SageError(n, "sage_jacobi_round_pairs")
    return [(int(pairs[2 * i]), int(pairs[2 * i + 1])) for i in range(n)]


def damped_solve_qr_f32(A, b, damp):
    A = _f32(A); b = _f32(b)
    x = np.zeros(b.shape[0], np.float32)
    _chk(lib().sage_damped_solve_qr_f32(_fp(A), _fp(b), b.shape[0], C.c_float(damp), _fp(x)), "sage_damped_solve_qr_f32")
    return x


def block_solve(packed, K, links, B, damp, diag_add=None, g_add=None):
    packed = np.ascontiguousarray(packed, dtype=np.float64)
    lk = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1))
    delta = np.zeros(K * B, np.float64)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    da = None if diag_add is None else np.ascontiguousarray(diag_add, np.float64)
    ga = None if g_add is None else np.ascontiguousarray(g_add, np.float64)
    _chk(lib().sage_block_solve(packed.ctypes.data_as(C.POINTER(C.c_double)), K, len(lk) // 2, lk.ctypes.data_as(C.POINTER(C.c_int32)), B,
                                C.c_double(damp), dp(da), dp(ga), delta.ctypes.data_as(C.POINTER(C.c_double))),
         "sage_block_solve")
    return delta


def block_covariance_raw(packed, K, nlinks, links, B, damp, diag_add, pairs, n_pairs, Sigma) -> int:
    """``sage_block_covariance`` with raw addresses (None -> NULL) -> status code"""
    f = lib().sage_block_covariance
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return f(packed, K, nlinks, links, B, damp, diag_add, pairs, n_pairs, Sigma)


def block_covariance(packed, K, links, B, damp, pairs, diag_add=None):
    """``sage_block_covariance``: the blocks ``pairs`` [n,2] (a keyframe with itself, or a link either way round) of the
    inverse of the damped system ``sage_block_solve`` factorises -> Sigma [n,B,B] (rows pairs[.,0], columns pairs[.,1])"""
    packed = np.ascontiguousarray(packed, dtype=np.float64)
    lk = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1))
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    da = None if diag_add is None else np.ascontiguousarray(diag_add, np.float64)
    Sigma = np.zeros((len(pr), B, B), np.float64)
    _chk(block_covariance_raw(packed.ctypes.data, K, len(lk) // 2, lk.ctypes.data, B, damp, None if da is None else da.ctypes.data,
                              pr.ctypes.data, len(pr), Sigma.ctypes.data), "sage_block_covariance")
    return Sigma


def covariance_plan(K, links):
    """``sage_covariance_plan``: (blocks the plan of K keyframes and ``links`` stores, blocks the covariance closure adds)"""
    lk = np.ascontiguousarray(np.asarray(links, dtype=np.int32).reshape(-1))
    stored, added = C.c_int32(), C.c_int32()
    f = lib().sage_covariance_plan
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(f(K, len(lk) // 2, lk.ctypes.data, C.addressof(stored), C.addressof(added)), "sage_covariance_plan")
    return stored.value, added.value


def solve_lookahead_count() -> int:
    f = lib().sage_solve_lookahead_count
    f.restype = C.c_longlong
    return int(f())


def block_solve_domains(packed, K, links, B, damp, ndomains, diag_add=None, g_add=None):
    """sage_block_solve by domain decomposition on `ndomains` host threads (long windows, loop closures)."""
    p = np.ascontiguousarray(packed, np.float64)
    lk = np.ascontiguousarray(np.asarray(links, np.int32).reshape(-1))
    out = np.zeros(K * B, np.float64)
    dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    da = None if diag_add is None else np.ascontiguousarray(diag_add, np.float64)
    ga = None if g_add is None else np.ascontiguousarray(g_add, np.float64)
    _chk(lib().sage_block_solve_domains(p.ctypes.data_as(C.POINTER(C.c_double)), K, len(links),
                                        lk.ctypes.data_as(C.POINTER(C.c_int32)), B, C.c_double(damp), dp(da), dp(ga),
                                        ndomains, out.ctypes.data_as(C.POINTER(C.c_double))), "sage_block_solve_domains")
    return out


def lm_config_default() -> SageLmConfig:
    cfg = SageLmConfig()
    lib().sage_lm_config_default(C.byref(cfg))
    return cfg


def pack_pose(R, t) -> np.ndarray:
    return np.concatenate([_f32(R).reshape(9), _f32(t).reshape(3)])


def track_lm(cfg: SageLmConfig, dof: int, lin_fn, err_fn, pose12, scale: float, trace_cap: int = 256):
    """Run the tracker LM policy (``camera_tracker.cpp:1156-1279``) with Python evaluation callbacks.
    ``lin_fn(pose12, scale) -> (AtA, Atb, error)``; ``err_fn(pose12, scale) -> error``."""
    def _lin(ctx, p, s, AtA, Atb, err):
        A, b, e = lin_fn(np.ctypeslib.as_array(p, (12,)).copy(), float(s))
        A = _f32(A).reshape(-1); b = _f32(b).reshape(-1)
        for i in range(dof * dof):
            AtA[i] = A[i]
        for i in range(dof):
            Atb[i] = b[i]
        err[0] = e
        return 0

    def _err(ctx, p, s, err):
        err[0] = err_fn(np.ctypeslib.as_array(p, (12,)).copy(), float(s))
        return 0

    pose = _f32(pose12).reshape(12).copy()
    sc = C.c_float(scale)
    fe = C.c_float(0); it = C.c_int(0); tl = C.c_int(0)
    trace = (SageLmTraceEntry * trace_cap)()
    cb1, cb2 = TRACK_LIN_FN(_lin), TRACK_ERR_FN(_err)
    _chk(lib().sage_track_lm(C.byref(cfg), dof, cb1, cb2, None, _fp(pose), C.byref(sc), C.byref(fe), C.byref(it),
                             trace, trace_cap, C.byref(tl)), "sage_track_lm")
    tr = [dict(damp=trace[i].damp, error=trace[i].error, candidate_error=trace[i].candidate_error,
               accepted=trace[i].accepted, relinearized=trace[i].relinearized) for i in range(tl.value)]
    return pose, sc.value, fe.value, it.value, tr


SAGE_TRACK_MAX_BATCH = 32
TRACK_BATCH_EVAL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float))


def _trace_dicts(tr, n):
    return [dict(damp=tr[i].damp, error=tr[i].error, candidate_error=tr[i].candidate_error, accepted=tr[i].accepted,
                 relinearized=tr[i].relinearized) for i in range(n)]


def track_lm_batch_raw(cfg_ptr, dof, B, eval_cb, pose_ptr, scale_ptr, err_ptr, iters_ptr, status_ptr, trace_ptr, trace_cap,
                       trace_len_ptr) -> int:
    """``sage_track_lm_batch`` with the arguments as given (pointers may be None) -> status code"""
    f = lib().sage_track_lm_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    return int(f(cfg_ptr, int(dof), int(B), C.cast(eval_cb, C.c_void_p) if eval_cb is not None else None, None, pose_ptr,
                 scale_ptr, err_ptr, iters_ptr, status_ptr, trace_ptr, int(trace_cap), trace_len_ptr))


def _batch_outputs(B, poses, scales, trace_cap):
    n = max(B, 1)
    p = np.zeros((n, 12), np.float32); s = np.ones(n, np.float32)
    if B:
        p[:B] = _f32(poses).reshape(B, 12); s[:B] = _f32(scales).reshape(B)
    return (p, s, np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32),
            (SageLmTraceEntry * (n * max(trace_cap, 1)))(), np.zeros(n, np.int32))


def _batch_result(rc, B, out, trace_cap):
    p, s, fe, it, st, tr, tl = out
    traces = [_trace_dicts((SageLmTraceEntry * max(trace_cap, 1)).from_buffer(tr, b * trace_cap * C.sizeof(SageLmTraceEntry)),
                           int(tl[b])) for b in range(B)]
    return rc, p[:B], s[:B], fe[:B], it[:B], st[:B], traces


def track_lm_batch(cfg: SageLmConfig, dof: int, eval_fn, poses, scales, trace_cap: int = 256):
    """B runs of the tracker LM policy in lock-step (``sage_track_lm_batch``).  ``eval_fn(problems, want_jac, poses [n,12],
    scales [n])`` is called once per round and returns one answer per request: ``(AtA, Atb, error)`` where want_jac, else
    ``error``.  poses [B,12], scales [B].  -> (rc, poses, scales, errors, iters, status, traces), arrays of B (float32 /
    int32), traces: B lists of dicts."""
    B = len(poses)

    def _eval(ctx, n, problem, want_jac, p, s, AtA, Atb, err):
        probs = [int(problem[i]) for i in range(n)]
        wj = [bool(want_jac[i]) for i in range(n)]
        ans = eval_fn(probs, wj, np.ctypeslib.as_array(p, (n, 12)).copy(), np.ctypeslib.as_array(s, (n,)).copy())
        for i in range(n):
            if wj[i]:
                A, b, e = ans[i]
                A = _f32(A).reshape(-1); b = _f32(b).reshape(-1)
                for k in range(dof * dof):
                    AtA[49 * i + k] = A[k]
                for k in range(dof):
                    Atb[7 * i + k] = b[k]
                err[i] = e
            else:
                err[i] = ans[i]
        return 0

    out = _batch_outputs(B, poses, scales, trace_cap)
    cb = TRACK_BATCH_EVAL_FN(_eval)
    rc = track_lm_batch_raw(C.addressof(cfg), dof, B, cb, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                            out[3].ctypes.data, out[4].ctypes.data, C.addressof(out[5]), trace_cap, out[6].ctypes.data)
    return _batch_result(rc, B, out, trace_cap)


# --------------------------------------------------------------------------- device side
def track_frame_batch_raw(cfg_ptr, dof, probs_ptr, B, pose_ptr, scale_ptr, err_ptr, iters_ptr, status_ptr, trace_ptr, trace_cap,
                          trace_len_ptr) -> int:
    """``sage_track_frame_batch`` with the arguments as given (pointers may be None) -> status code"""
    f = lib().sage_track_frame_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    return int(f(cfg_ptr, int(dof), probs_ptr, int(B), pose_ptr, scale_ptr, err_ptr, iters_ptr, status_ptr, trace_ptr,
                 int(trace_cap), trace_len_ptr))


def track_frame_batch(cfg: SageLmConfig, dof: int, probs, poses, scales, trace_cap: int = 256):
    """``sage_track_frame_batch``: B ``SageTrackProblem`` s tracked in lock-step on the HIP kernels.  poses [B,12], scales [B].
    -> (rc, poses, scales, errors, iters, status, traces) as ``track_lm_batch``; row b is what ``track_frame`` returns for
    probs[b], bit for bit."""
    B = len(probs)
    arr = (SageTrackProblem * max(B, 1))(*probs)
    out = _batch_outputs(B, poses, scales, trace_cap)
    rc = track_frame_batch_raw(C.addressof(cfg), dof, C.addressof(arr), B, out[0].ctypes.data, out[1].ctypes.data,
                               out[2].ctypes.data, out[3].ctypes.data, out[4].ctypes.data, C.addressof(out[5]), trace_cap,
                               out[6].ctypes.data)
    return _batch_result(rc, B, out, trace_cap)


def track_frame(cfg: SageLmConfig, dof: int, prob: "SageTrackProblem", pose12, scale: float, trace_cap: int = 256):
    """sage_track_frame: the tracker LM wired to the HIP kernels.  Returns (rc, pose12, scale, final_error, iters, trace)."""
    L = lib()
    p = _f32(pose12).copy()
    sc = C.c_float(scale); fe = C.c_float(); it = C.c_int(); tl = C.c_int()
    tr = (SageLmTraceEntry * trace_cap)()
    rc = L.sage_track_frame(C.byref(cfg), dof, C.byref(prob), _fp(p), C.byref(sc), C.byref(fe), C.byref(it), tr,
                            trace_cap, C.byref(tl))
    trace = [dict(damp=tr[i].damp, error=tr[i].error, candidate_error=tr[i].candidate_error,
                  accepted=tr[i].accepted, relinearized=tr[i].relinearized) for i in range(tl.value)]
    return rc, p, sc.value, fe.value, it.value, trace


class SageOverlapStats(C.Structure):
    _fields_ = [("input_area", C.c_double), ("warp_area", C.c_double), ("area_ratio", C.c_float),
                ("inlier_ratio", C.c_float), ("average_motion", C.c_float), ("n_points", C.c_int32),
                ("n_pos_depth", C.c_int32), ("n_in_mask", C.c_int32), ("n_candidates", C.c_int32 * 2)]


def track_overlap_raw(ws_handle, R, t, dpts0_ptr, depth_scale, homo_ptr, M, cam_ptr, mask_ptr, eps, out_ptr) -> int:
    """``sage_track_overlap`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_track_overlap
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                  C.c_float, C.c_void_p]
    return int(f(ws_handle, R, t, dpts0_ptr, depth_scale, homo_ptr, int(M), cam_ptr, mask_ptr, eps, out_ptr))


def track_overlap(ws: "Workspace", R, t, dpts0, homo, cam, mask, eps, depth_scale: float = 1.0) -> SageOverlapStats:
    """``CameraTracker::ComputeAreaInlierRatio`` through ``sage_track_overlap``.  R [3,3], t [3]: host arrays; dpts0 [M],
    homo [M,3], mask [h,w]: contiguous float32 cuda tensors; cam: anything with fx, fy, cx, cy, w, h."""
    Rh = _f32(R).reshape(9); th = _f32(t).reshape(3)
    c = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    M = int(homo.shape[0])
    assert dpts0.numel() == M and tuple(mask.shape) == (int(c.h), int(c.w))
    out = SageOverlapStats()
    _chk(track_overlap_raw(ws.h, Rh.ctypes.data, th.ctypes.data, dptr(dpts0), float(depth_scale), dptr(homo), M,
                           C.addressof(c), dptr(mask), float(eps), C.addressof(out)), "sage_track_overlap")
    return out


OVERLAP_MAX_BATCH = 32


class SageOverlapPose(C.Structure):
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("depth_scale", C.c_float)]


def overlap_pose(R, t, depth_scale: float = 1.0) -> SageOverlapPose:
    """R [3,3] (row-major R10), t [3], depth_scale -> one row of ``sage_track_overlap_batch``"""
    return SageOverlapPose((C.c_float * 9)(*_f32(R).reshape(9)), (C.c_float * 3)(*_f32(t).reshape(3)), float(depth_scale))


def track_overlap_batch_raw(ws_handle, poses_ptr, B, dpts0_ptr, homo_ptr, M, cam_ptr, mask_ptr, eps, out_ptr) -> int:
    """``sage_track_overlap_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_track_overlap_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                  C.c_void_p]
    return int(f(ws_handle, poses_ptr, int(B), dpts0_ptr, homo_ptr, int(M), cam_ptr, mask_ptr, eps, out_ptr))


def track_overlap_batch(ws: "Workspace", poses, dpts0, homo, cam, mask, eps) -> list:
    """``sage_track_overlap`` for every pose of ``poses`` (``SageOverlapPose``, or (R, t, depth_scale) triples) over one
    point set, camera and mask, in three launches and one wait -> a list of ``SageOverlapStats``, row b what the single
    call returns for poses[b], byte for byte."""
    rows = [p if isinstance(p, SageOverlapPose) else overlap_pose(*p) for p in poses]
    B = len(rows)
    arr = (SageOverlapPose * max(B, 1))(*rows)
    c = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    M = int(homo.shape[0])
    assert dpts0.numel() == M and tuple(mask.shape) == (int(c.h), int(c.w))
    out = (SageOverlapStats * max(B, 1))()
    _chk(track_overlap_batch_raw(ws.h, C.addressof(arr), B, dptr(dpts0), dptr(homo), M, C.addressof(c), dptr(mask),
                                 float(eps), C.addressof(out)), "sage_track_overlap_batch")
    return [out[b] for b in range(B)]


def track_overlap_batch_plan_raw(M, B, device_bytes_ptr, pinned_bytes_ptr, launches_ptr, workgroups_ptr) -> int:
    f = lib().sage_track_overlap_batch_plan
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(int(M), int(B), device_bytes_ptr, pinned_bytes_ptr, launches_ptr, workgroups_ptr))


def track_overlap_batch_plan(M: int, B: int) -> dict:
    """What a batch of B poses over M points reserves and launches, through ``sage_track_overlap_batch_plan`` (host only)."""
    dev = C.c_int64(); pin = C.c_int64(); launches = C.c_int32(); wgs = C.c_int32()
    _chk(track_overlap_batch_plan_raw(M, B, C.addressof(dev), C.addressof(pin), C.addressof(launches), C.addressof(wgs)),
         "sage_track_overlap_batch_plan")
    return dict(device_bytes=dev.value, pinned_bytes=pin.value, launches=launches.value, workgroups_per_row=wgs.value)


def track_overlap_batch_launches(ws: "Workspace") -> int:
    """kernel launches of the workspace's last ``sage_track_overlap_batch``"""
    f = lib().sage_track_overlap_batch_launches
    f.argtypes = [C.c_void_p]
    return int(f(ws.h if ws is not None else None))


def convex_hull_area(xy):
    """``sage_convex_hull_area`` of [n,2] points -> (area, n_vertices)"""
    p = _f32(xy).reshape(-1, 2)
    area = C.c_double(); nv = C.c_int()
    _chk(lib().sage_convex_hull_area(_fp(p), int(p.shape[0]), C.byref(area), C.byref(nv)), "sage_convex_hull_area")
    return area.value, nv.value


class SageDepthScaleStats(C.Structure):
    _fields_ = [("ratio", C.c_float), ("n_points", C.c_int32), ("n_pos_depth", C.c_int32), ("n_selected", C.c_int32),
                ("n_nan", C.c_int32), ("n_used", C.c_int32)]


def depth_scale_ratio_raw(ws_handle, R10, t10, dpt0_ptr, loc_ptr, homo_ptr, M, cam_ptr, bias1_ptr, mask_ptr, eps, drop_nan,
                          ratios_ptr, selected_ptr, out_ptr) -> int:
    """``sage_depth_scale_ratio`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_depth_scale_ratio
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(ws_handle, R10, t10, dpt0_ptr, loc_ptr, homo_ptr, int(M), cam_ptr, bias1_ptr, mask_ptr, eps, int(drop_nan),
                 ratios_ptr, selected_ptr, out_ptr))


def depth_scale_ratio(ws: "Workspace", R10, t10, dpt0, homo0, cam, bias1, mask, eps, drop_nan: bool = False, loc1d0=None,
                      per_point: bool = False):
    """``Mapper::CorrectDepthScale`` (``drop_nan`` False) / the loop detector's ``df::CorrectDepthScale`` (True) through
    ``sage_depth_scale_ratio``.  R10 [3,3], t10 [3]: host arrays; homo0 [M,3], bias1 [h,w], mask [h,w]: contiguous float32
    cuda tensors; dpt0: keyframe 0's depth map [h,w] with ``loc1d0`` [M] (int64 cuda tensor), or the M gathered depths
    without.  -> ``SageDepthScaleStats``, or with ``per_point`` (stats, ratios [M] float32, selected [M] int32) -- the last
    two cuda tensors."""
    import torch
    Rh = _f32(R10).reshape(9); th = _f32(t10).reshape(3)
    c = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    M = int(homo0.shape[0])
    hw = (int(c.h), int(c.w))
    assert tuple(mask.shape) == hw and tuple(bias1.shape) == hw
    if loc1d0 is None:
        assert dpt0.numel() == M
    else:
        assert loc1d0.dtype == torch.int64 and loc1d0.numel() == M and dpt0.numel() == hw[0] * hw[1]
    ratios = torch.empty(M, dtype=torch.float32, device=homo0.device) if per_point else None
    selected = torch.empty(M, dtype=torch.int32, device=homo0.device) if per_point else None
    out = SageDepthScaleStats()
    _chk(depth_scale_ratio_raw(ws.h, Rh.ctypes.data, th.ctypes.data, dptr(dpt0), dptr(loc1d0), dptr(homo0), M, C.addressof(c),
                               dptr(bias1), dptr(mask), float(eps), int(bool(drop_nan)), dptr(ratios), dptr(selected),
                               C.addressof(out)), "sage_depth_scale_ratio")
    return (out, ratios, selected) if per_point else out


def median_f32_raw(ws_handle, values_ptr, loc_ptr, n, drop_nan, median_ptr, n_used_ptr, n_nan_ptr) -> int:
    """``sage_median_f32`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_median_f32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(ws_handle, values_ptr, loc_ptr, int(n), int(drop_nan), median_ptr, n_used_ptr, n_nan_ptr))


def median_f32(ws: "Workspace", values, loc1d=None, drop_nan: bool = False):
    """``torch::median`` (the lower median) of a contiguous float32 cuda tensor, or of ``values[loc1d]`` (int64 cuda tensor),
    through ``sage_median_f32`` -> (median as np.float32, n_used, n_nan)"""
    import torch
    assert values.dtype == torch.float32
    n = int(values.numel())
    if loc1d is not None:
        assert loc1d.dtype == torch.int64
        n = int(loc1d.numel())
    med = C.c_float(); n_used = C.c_int(); n_nan = C.c_int()
    _chk(median_f32_raw(ws.h, dptr(values), dptr(loc1d), n, int(bool(drop_nan)), C.addressof(med), C.addressof(n_used),
                        C.addressof(n_nan)), "sage_median_f32")
    return np.float32(med.value), n_used.value, n_nan.value


DEPTH_SCALE_MAX_BATCH = 32


class SageDepthScaleRow(C.Structure):
    _fields_ = [("R10", C.c_float * 9), ("t10", C.c_float * 3), ("dpt0_dev", C.c_void_p), ("loc1d0_dev", C.c_void_p),
                ("homo0_dev", C.c_void_p), ("M", C.c_int32), ("ratios_out_dev", C.c_void_p), ("selected_out_dev", C.c_void_p)]


def depth_scale_ratio_batch_raw(ws_handle, rows_ptr, B, cam_ptr, bias1_ptr, mask_ptr, eps, drop_nan, out_ptr) -> int:
    """``sage_depth_scale_ratio_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_depth_scale_ratio_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    return int(f(ws_handle, rows_ptr, int(B), cam_ptr, bias1_ptr, mask_ptr, eps, int(drop_nan), out_ptr))


def depth_scale_row(R10, t10, dpt0, homo0, loc1d0=None, ratios=None, selected=None, M=None) -> SageDepthScaleRow:
    """One row of a depth-scale batch from host R10 [3,3], t10 [3] and cuda tensors as in ``depth_scale_ratio``; ``M``: only
    the first M points of ``homo0`` (and of ``loc1d0`` / the gathered ``dpt0``)"""
    r = SageDepthScaleRow()
    r.R10[:] = [float(v) for v in _f32(R10).reshape(9)]
    r.t10[:] = [float(v) for v in _f32(t10).reshape(3)]
    r.dpt0_dev, r.loc1d0_dev, r.homo0_dev = dptr(dpt0).value, dptr(loc1d0).value, dptr(homo0).value
    r.M = int(homo0.shape[0]) if M is None else int(M)
    r.ratios_out_dev, r.selected_out_dev = dptr(ratios).value, dptr(selected).value
    return r


def depth_scale_ratio_batch(ws: "Workspace", rows, cam, bias1, mask, eps, drop_nan: bool = False) -> list:
    """``sage_depth_scale_ratio`` for every row of ``rows`` (``SageDepthScaleRow``: ``depth_scale_row``) against one keyframe
    to scale (camera, bias, mask), in five launches and one wait -> a list of ``SageDepthScaleStats``, row b what the
    single call returns on that row's inputs, byte for byte.  The caller keeps the rows' tensors alive."""
    B = len(rows)
    arr = (SageDepthScaleRow * max(B, 1))(*rows)
    c = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    hw = (int(c.h), int(c.w))
    assert tuple(mask.shape) == hw and tuple(bias1.shape) == hw
    out = (SageDepthScaleStats * max(B, 1))()
    _chk(depth_scale_ratio_batch_raw(ws.h, C.addressof(arr), B, C.addressof(c), dptr(bias1), dptr(mask), float(eps),
                                     int(bool(drop_nan)), C.addressof(out)), "sage_depth_scale_ratio_batch")
    return [out[b] for b in range(B)]


def median_f32_batch_raw(ws_handle, values_ptr, loc_ptr, n_ptr, B, drop_nan, median_ptr, n_used_ptr, n_nan_ptr) -> int:
    """``sage_median_f32_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_median_f32_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(ws_handle, values_ptr, loc_ptr, n_ptr, int(B), int(drop_nan), median_ptr, n_used_ptr, n_nan_ptr))


def median_f32_batch(ws: "Workspace", values, loc1d=None, drop_nan: bool = False) -> list:
    """``median_f32`` of every tensor of ``values`` (``loc1d``: None, or a list with an int64 cuda tensor or None per
    segment) through ``sage_median_f32_batch``: five launches, one wait -> a list of (median as np.float32, n_used, n_nan)"""
    import torch
    B = len(values)
    locs = list(loc1d) if loc1d is not None else [None] * B
    assert len(locs) == B and all(v.dtype == torch.float32 for v in values)
    vp = (C.c_void_p * max(B, 1))(*[dptr(v).value for v in values])
    lp = (C.c_void_p * max(B, 1))(*[dptr(l).value for l in locs])
    n = (C.c_int32 * max(B, 1))(*[int(v.numel() if l is None else l.numel()) for v, l in zip(values, locs)])
    med = (C.c_float * max(B, 1))(); n_used = (C.c_int32 * max(B, 1))(); n_nan = (C.c_int32 * max(B, 1))()
    _chk(median_f32_batch_raw(ws.h, C.addressof(vp), C.addressof(lp) if loc1d is not None else None, C.addressof(n), B,
                              int(bool(drop_nan)), C.addressof(med), C.addressof(n_used), C.addressof(n_nan)),
         "sage_median_f32_batch")
    return [(np.float32(med[b]), n_used[b], n_nan[b]) for b in range(B)]


def depth_scale_ratio_batch_plan_raw(M_ptr, B, device_bytes_ptr, pinned_bytes_ptr, launches_ptr, workgroups_ptr) -> int:
    f = lib().sage_depth_scale_ratio_batch_plan
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(M_ptr, int(B), device_bytes_ptr, pinned_bytes_ptr, launches_ptr, workgroups_ptr))


def depth_scale_ratio_batch_plan(M) -> dict:
    """What a batch of len(M) rows of M[b] points reserves and launches, through ``sage_depth_scale_ratio_batch_plan`` (host
    only)."""
    B = len(M)
    arr = (C.c_int32 * max(B, 1))(*[int(m) for m in M])
    dev = C.c_int64(); pin = C.c_int64(); launches = C.c_int32(); wgs = C.c_int32()
    _chk(depth_scale_ratio_batch_plan_raw(C.addressof(arr), B, C.addressof(dev), C.addressof(pin), C.addressof(launches),
                                          C.addressof(wgs)), "sage_depth_scale_ratio_batch_plan")
    return dict(device_bytes=dev.value, pinned_bytes=pin.value, launches=launches.value, workgroups=wgs.value)


def depth_scale_ratio_batch_launches(ws: "Workspace") -> int:
    """kernel launches of the workspace's last ``sage_depth_scale_ratio_batch`` or ``sage_median_f32_batch``"""
    f = lib().sage_depth_scale_ratio_batch_launches
    f.argtypes = [C.c_void_p]
    return int(f(ws.h if ws is not None else None))


class Workspace:
    """``SageWorkspace``: stream + scratch of one host thread."""

    def __init__(self, stream=None):
        self.h = C.c_void_p()
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
        _chk(lib().sage_workspace_create(sp, C.byref(self.h)), "sage_workspace_create")

    def close(self):
        if self.h:
            lib().sage_workspace_destroy(self.h)
            self.h = C.c_void_p()

    def set_registration_finish(self, mode: int):
        """where this workspace's registrations run their finish: ``SAGE_REG_FINISH_HOST`` (the default) or
        ``SAGE_REG_FINISH_DEVICE`` (``sage_workspace_set_registration_finish``)"""
        _chk(workspace_set_registration_finish_raw(self.h, mode), "sage_workspace_set_registration_finish")

    def registration_finish(self) -> int:
        return workspace_registration_finish_raw(self.h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------- the loop detector's bag of words
SAGE_BOW_L1, SAGE_BOW_L2, SAGE_BOW_CHI_SQUARE, SAGE_BOW_KL, SAGE_BOW_BHATTACHARYYA, SAGE_BOW_DOT_PRODUCT = range(6)


class SageVocabularyDesc(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("C", C.c_int32), ("parent", C.c_void_p), ("descriptors", C.c_void_p),
                ("weight", C.c_void_p), ("word_id", C.c_void_p), ("scoring", C.c_int32)]


class SageBowStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_points", "n_words", "n_leaves_hit", "n_zero_weight", "n_inner_nodes_hit")]


def vocabulary_create_raw(parent, descriptors, weight, word_id, scoring=SAGE_BOW_L1):
    """``sage_vocabulary_create`` on host arrays as given (parent [n] int32, descriptors [n, C] float32, weight [n] float64,
    word_id [n] int32) -> (status code, handle)"""
    parent = np.ascontiguousarray(parent, np.int32); word_id = np.ascontiguousarray(word_id, np.int32)
    descriptors = np.ascontiguousarray(descriptors, np.float32); weight = np.ascontiguousarray(weight, np.float64)
    n = int(parent.shape[0])
    assert descriptors.ndim == 2 and descriptors.shape[0] == n and weight.shape == (n,) and word_id.shape == (n,)
    d = SageVocabularyDesc(n, int(descriptors.shape[1]), parent.ctypes.data, descriptors.ctypes.data, weight.ctypes.data,
                           word_id.ctypes.data, int(scoring))
    h = C.c_void_p()
    f = lib().sage_vocabulary_create
    f.argtypes = [C.c_void_p, C.c_void_p]
    return int(f(C.addressof(d), C.addressof(h))), h


class Vocabulary:
    """``SageVocabulary``: the vocabulary tree on the device, immutable; ``voc`` is a dict with parent, descriptors, weight,
    word_id (and optionally scoring) as ``vocabulary.load_opencv_yaml`` and ``synth.make_vocabulary`` return it."""

    def __init__(self, voc: dict):
        rc, self.h = vocabulary_create_raw(voc["parent"], voc["descriptors"], voc["weight"], voc["word_id"],
                                           voc.get("scoring", SAGE_BOW_L1))
        _chk(rc, "sage_vocabulary_create")
        L = lib()
        for name in ("num_nodes", "num_words", "channels", "depth", "max_fanout", "staged_nodes"):
            fn = getattr(L, "sage_vocabulary_" + name)
            fn.argtypes = [C.c_void_p]
            setattr(self, name, int(fn(self.h)))

    def close(self):
        if self.h:
            f = lib().sage_vocabulary_destroy
            f.argtypes = [C.c_void_p]; f.restype = None
            f(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bow_transform_raw(ws_handle, voc_handle, desc_ptr, loc_ptr, M, P, ids_ptr, vals_ptr, capacity, word_out_ptr, out_ptr) -> int:
    """``sage_bow_transform`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_bow_transform
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                  C.c_void_p]
    return int(f(ws_handle, voc_handle, desc_ptr, loc_ptr, int(M), int(P), ids_ptr, vals_ptr, int(capacity), word_out_ptr, out_ptr))


def bow_transform(ws: "Workspace", voc: Vocabulary, desc, loc1d=None, per_point: bool = False):
    """``TemplatedTensorVocabulary::transform`` of ``LoopDetector::AddKeyframe`` through ``sage_bow_transform``.  desc: a
    contiguous float32 cuda tensor [C, P] (``feat_desc`` reshaped) read at ``loc1d`` [M] (int64 cuda tensor), or [C, M]
    already gathered without.  -> (word ids int32 [n], values float64 [n], ``SageBowStats``) and, with ``per_point``, the
    word of every point (int32 cuda tensor [M])."""
    import torch
    assert desc.dtype == torch.float32 and desc.dim() == 2 and int(desc.shape[0]) == voc.channels
    P = int(desc.shape[1])
    M = P if loc1d is None else int(loc1d.numel())
    assert loc1d is None or loc1d.dtype == torch.int64
    cap = min(M, voc.num_words)
    ids = np.empty(cap, np.int32); vals = np.empty(cap, np.float64)
    words = torch.empty(M, dtype=torch.int32, device=desc.device) if per_point else None
    out = SageBowStats()
    _chk(bow_transform_raw(ws.h, voc.h, dptr(desc), dptr(loc1d), M, P, ids.ctypes.data, vals.ctypes.data, cap, dptr(words),
                           C.addressof(out)), "sage_bow_transform")
    r = (ids[:out.n_words].copy(), vals[:out.n_words].copy(), out)
    return r + (words,) if per_point else r


# --------------------------------------------------------------------------- training the vocabulary
SAGE_VOC_TF_IDF, SAGE_VOC_TF, SAGE_VOC_IDF, SAGE_VOC_BINARY = range(4)
SAGE_VOC_BUILD_MAX_LEVELS = 8


class SageVocabularyBuildConfig(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32),
                ("max_iterations", C.c_int32), ("seed", C.c_uint64)]


class SageVocabularyBuildStats(C.Structure):
    _fields_ = [("levels", C.c_int32), ("n_nodes", C.c_int32), ("n_words", C.c_int32), ("nodes_capped", C.c_int32)] + \
               [(n, C.c_int32 * SAGE_VOC_BUILD_MAX_LEVELS) for n in ("nodes", "kmeans_nodes", "seed_rounds", "rounds", "launches", "waits")]


def vocabulary_build_config_default() -> SageVocabularyBuildConfig:
    cfg = SageVocabularyBuildConfig()
    f = lib().sage_vocabulary_build_config_default
    f.argtypes = [C.c_void_p]; f.restype = None
    f(C.addressof(cfg))
    return cfg


def vocabulary_build_draw(seed: int, path, j: int) -> int:
    """``sage_vocabulary_build_draw``: draw j of the node at ``path`` (child indices from the root).  No device."""
    path = np.ascontiguousarray(path, np.int32)
    f = lib().sage_vocabulary_build_draw
    f.argtypes = [C.c_uint64, C.c_void_p, C.c_int, C.c_int]; f.restype = C.c_uint64
    return int(f(int(seed), path.ctypes.data if path.size else None, int(path.size), int(j)))


def vocabulary_build_plan_raw(Cn, M, k, L):
    """``sage_vocabulary_build_plan`` -> (status code, dict(device_bytes, pinned_bytes, launches_per_seed_round,
    launches_per_lloyd_round)).  No device."""
    db, pb = C.c_int64(-1), C.c_int64(-1)
    ls, ll = C.c_int32(-1), C.c_int32(-1)
    f = lib().sage_vocabulary_build_plan
    f.argtypes = [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = int(f(int(Cn), int(M), int(k), int(L), C.addressof(db), C.addressof(pb), C.addressof(ls), C.addressof(ll)))
    return rc, dict(device_bytes=db.value, pinned_bytes=pb.value, launches_per_seed_round=ls.value, launches_per_lloyd_round=ll.value)


def vocabulary_build_raw(ws_handle, cfg_ptr, desc_ptr, Cn, M, doc_begin_ptr, n_docs, out_ptr) -> int:
    """``sage_vocabulary_build`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_vocabulary_build
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]
    return int(f(ws_handle, cfg_ptr, desc_ptr, int(Cn), int(M), doc_begin_ptr, int(n_docs), out_ptr))


class VocabularyBuild:
    """``sage_vocabulary_build``: hierarchical k-means over ``desc`` (float32 cuda tensor [C, M], channel-major) whose
    documents are the column ranges ``doc_begin`` [n_docs + 1].  Keyword arguments set ``SageVocabularyBuildConfig`` fields
    (k, L, weighting, scoring, max_iterations, seed).
    ``voc``: the finished tree as ``Vocabulary`` / ``vocabulary.save_opencv_yaml`` take it (host copies); ``docs_with_word``
    [n_words]; ``stats``; ``node_of_point()``: int32 cuda tensor [M] (a copy), the leaf node of every training point."""

    def __init__(self, ws: "Workspace", desc, doc_begin, **cfg_fields):
        import torch
        assert desc.dtype == torch.float32 and desc.dim() == 2
        cfg = vocabulary_build_config_default()
        for name, v in cfg_fields.items():
            assert hasattr(cfg, name), name
            setattr(cfg, name, int(v))
        doc_begin = np.ascontiguousarray(doc_begin, np.int64)
        self.M = int(desc.shape[1])
        self.h = C.c_void_p()
        _chk(vocabulary_build_raw(ws.h, C.addressof(cfg), dptr(desc), int(desc.shape[0]), self.M, doc_begin.ctypes.data,
                                  doc_begin.size - 1, C.addressof(self.h)), "sage_vocabulary_build")
        L = lib()
        d = SageVocabularyDesc()
        f = L.sage_vocabulary_build_desc; f.argtypes = [C.c_void_p, C.c_void_p]
        _chk(int(f(self.h, C.addressof(d))), "sage_vocabulary_build_desc")
        n, Cn = int(d.n_nodes), int(d.C)

        def arr(ptr, count, ctype, dtype):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (count,)).astype(dtype, copy=True)

        word_id = arr(d.word_id, n, C.c_int32, np.int32)
        self.voc = dict(parent=arr(d.parent, n, C.c_int32, np.int32), descriptors=arr(d.descriptors, n * Cn, C.c_float, np.float32).reshape(n, Cn),
                        weight=arr(d.weight, n, C.c_double, np.float64), word_id=word_id, k=int(cfg.k), L=int(cfg.L),
                        scoring=int(d.scoring), weighting=int(cfg.weighting), n_nodes=n, n_words=int((word_id >= 0).sum()), C=Cn)
        ni, nw = C.c_void_p(), C.c_int()
        f = L.sage_vocabulary_build_docs_with_word; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(int(f(self.h, C.addressof(ni), C.addressof(nw))), "sage_vocabulary_build_docs_with_word")
        self.docs_with_word = arr(ni, nw.value, C.c_int32, np.int32) if nw.value else np.zeros(0, np.int32)
        self.stats = SageVocabularyBuildStats()
        f = L.sage_vocabulary_build_stats; f.argtypes = [C.c_void_p, C.c_void_p]
        _chk(int(f(self.h, C.addressof(self.stats))), "sage_vocabulary_build_stats")

    def node_of_point(self):
        p = C.c_void_p()
        f = lib().sage_vocabulary_build_node_of_point; f.argtypes = [C.c_void_p, C.c_void_p]
        _chk(int(f(self.h, C.addressof(p))), "sage_vocabulary_build_node_of_point")
        import torch

        class _Holder:
            pass

        view = _Holder()
        view.__cuda_array_interface__ = dict(shape=(self.M,), typestr="<i4", data=(int(p.value), False), version=2)
        return torch.as_tensor(view, device="cuda").clone()

    def close(self):
        if self.h:
            f = lib().sage_vocabulary_build_destroy
            f.argtypes = [C.c_void_p]; f.restype = None
            f(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _bow_vec(ids, vals):
    ids = np.ascontiguousarray(ids, np.int32); vals = np.ascontiguousarray(vals, np.float64)
    assert ids.ndim == 1 and ids.shape == vals.shape
    return ids, vals


def bow_score_raw(ids1, vals1, ids2, vals2):
    """``sage_bow_score`` -> (status code, score)"""
    ids1, vals1 = _bow_vec(ids1, vals1); ids2, vals2 = _bow_vec(ids2, vals2)
    f = lib().sage_bow_score
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    s = C.c_double(float("nan"))
    rc = int(f(ids1.ctypes.data, vals1.ctypes.data, len(ids1), ids2.ctypes.data, vals2.ctypes.data, len(ids2), C.addressof(s)))
    return rc, s.value


def bow_score(ids1, vals1, ids2, vals2) -> float:
    """``L1Scoring::score`` of two bag-of-words vectors (ascending word ids) through ``sage_bow_score``"""
    rc, s = bow_score_raw(ids1, vals1, ids2, vals2)
    _chk(rc, "sage_bow_score")
    return s


class BowDatabase:
    """``SageBowDatabase``: DBoW2's inverted-file database with L1 scoring (host only)."""

    def __init__(self, n_words: int):
        self.h = C.c_void_p()
        f = lib().sage_bow_db_create
        f.argtypes = [C.c_int, C.c_void_p]
        _chk(int(f(int(n_words), C.addressof(self.h))), "sage_bow_db_create")

    def add_raw(self, ids, vals) -> int:
        """-> the entry id, or a negative status code"""
        ids, vals = _bow_vec(ids, vals)
        f = lib().sage_bow_db_add
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        return int(f(self.h, ids.ctypes.data, vals.ctypes.data, len(ids)))

    def add(self, ids, vals) -> int:
        e = self.add_raw(ids, vals)
        if e < 0:
            raise SageError(e, "sage_bow_db_add")
        return e

    def __len__(self) -> int:
        f = lib().sage_bow_db_size
        f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def query_raw(self, ids, vals, max_results: int = 0, max_id: int = -1, capacity: Optional[int] = None):
        """-> (status code, entry ids int32 [n], scores float64 [n], n as the library reported it)"""
        ids, vals = _bow_vec(ids, vals)
        cap = len(self) if capacity is None else int(capacity)
        entries = np.empty(max(cap, 1), np.int32); scores = np.empty(max(cap, 1), np.float64)
        n = C.c_int(-1)
        f = lib().sage_bow_db_query
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        rc = int(f(self.h, ids.ctypes.data, vals.ctypes.data, len(ids), int(max_results), int(max_id), entries.ctypes.data,
                   scores.ctypes.data, cap, C.addressof(n)))
        k = n.value if rc == 0 else 0
        return rc, entries[:k].copy(), scores[:k].copy(), n.value

    def query(self, ids, vals, max_results: int = 0, max_id: int = -1):
        """``TemplatedDatabase::query`` -> (entry ids, scores), best first, ties by ascending entry id"""
        rc, entries, scores, _ = self.query_raw(ids, vals, max_results, max_id)
        _chk(rc, "sage_bow_db_query")
        return entries, scores

    def close(self):
        if self.h:
            f = lib().sage_bow_db_destroy
            f.argtypes = [C.c_void_p]; f.restype = None
            f(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _dev(x, dtype=None):
    import torch
    if isinstance(x, torch.Tensor):
        return x.contiguous()
    a = np.ascontiguousarray(x, dtype=dtype)
    return torch.from_numpy(a).cuda()


class DeviceKeyframe:
    """device-resident copy of a synthetic/real keyframe in the reference layouts (a10)."""

    def __init__(self, kf, H, W):
        import torch
        self.feat_pyr = _dev(kf.feat_pyr, np.float32)
        self.grad_pyr = _dev(kf.grad_pyr, np.float32)
        self.bias = _dev(kf.bias, np.float32)
        self.basis = _dev(kf.basis, np.float32)
        self.loc1d = _dev(kf.loc1d, np.int64)
        self.loc1d_i32 = self.loc1d.to(torch.int32)
        self.homo = _dev(kf.homo, np.float32)
        self.N = int(self.homo.shape[0])
        self.H, self.W = H, W

    def view(self) -> SageKeyframeView:
        return SageKeyframeView(self.feat_pyr.data_ptr(), self.grad_pyr.data_ptr(), self.bias.data_ptr(),
                                self.basis.data_ptr(), self.loc1d.data_ptr(), self.homo.data_ptr(), self.N)


# --------------------------------------------------------------------------- prepared keyframes
SAGE_PREPARE_MAX_BATCH = 64
SAGE_PREP_PACKED, SAGE_PREP_LOC, SAGE_PREP_HOMO, SAGE_PREP_F0S = 0, 1, 2, 3


class SagePreparedInfo(C.Structure):
    _fields_ = [("N", C.c_int32), ("slots", C.c_int32), ("ordered", C.c_int32), ("padded", C.c_int32), ("refs", C.c_int32),
                ("device_bytes", C.c_uint64)]


class SageWindowBuildStats(C.Structure):
    _fields_ = [("keyframes", C.c_int32), ("prepared", C.c_int32), ("repacked", C.c_int32), ("ordered", C.c_int32),
                ("presampled", C.c_int32), ("launches", C.c_int32)]


def prepare_config(win) -> SageWindowConfig:
    """what a prepare call reads of a window's configuration (pyr, FS, photo_weights; CS rides along), from a
    ``synth.make_window`` window"""
    cfg = SageWindowConfig()
    cfg.pyr = make_pyramid(win.cams[0], win.L)
    cfg.FS, cfg.CS = win.FS, win.CS
    for l in range(win.L):
        cfg.photo_weights[l] = float(win.photo_weights[l])
    return cfg


def keyframe_prepare_batch_raw(ws_handle, cfg_ptr, views_ptr, B, out_ptr) -> int:
    """``sage_keyframe_prepare_batch`` with its arguments as given (NULL / 0 included) -> status code"""
    f = lib().sage_keyframe_prepare_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return int(f(ws_handle, cfg_ptr, views_ptr, B, out_ptr))


def keyframe_prepare_plan_raw(cfg_ptr, N_ptr, B, device_bytes_ptr, scratch_ptr, launches_ptr, waits_ptr) -> int:
    f = lib().sage_keyframe_prepare_plan
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    return int(f(cfg_ptr, N_ptr, B, device_bytes_ptr, scratch_ptr, launches_ptr, waits_ptr))


def keyframe_prepare_plan(cfg: SageWindowConfig, N) -> dict:
    """``sage_keyframe_prepare_plan`` (host only): per keyframe the bytes of its handle's allocation, the call's scratch on the
    workspace, and the launches and waits of a batch without a tile-padded keyframe (one more of each with one)"""
    n = np.ascontiguousarray(N, dtype=np.int32).reshape(-1)
    dev = np.zeros(max(1, n.size), dtype=np.uint64)
    scratch, launches, waits = C.c_uint64(0), C.c_int(0), C.c_int(0)
    _chk(keyframe_prepare_plan_raw(C.byref(cfg), n.ctypes.data, int(n.size), dev.ctypes.data, C.byref(scratch),
                                   C.byref(launches), C.byref(waits)), "sage_keyframe_prepare_plan")
    return dict(device_bytes=[int(x) for x in dev[:n.size]], scratch_bytes=int(scratch.value), launches=int(launches.value),
                waits=int(waits.value))


def keyframe_prepare_launches(ws: "Workspace") -> int:
    f = lib().sage_keyframe_prepare_launches
    f.argtypes = [C.c_void_p]
    return int(f(ws.h))


def keyframe_config_matches(a: SageWindowConfig, b: SageWindowConfig) -> bool:
    """would a keyframe prepared under ``a`` be taken by a window of ``b``?  (pyr, FS, photo_weights, bit for bit)"""
    f = lib().sage_keyframe_config_matches
    f.argtypes = [C.c_void_p, C.c_void_p]
    r = int(f(C.byref(a), C.byref(b)))
    if r < 0:
        raise SageError(r, "sage_keyframe_config_matches")
    return r == 1


def keyframe_info_raw(handle) -> SagePreparedInfo:
    """``sage_keyframe_info`` of a raw handle (a window may keep a handle alive whose caller has released it)"""
    f = lib().sage_keyframe_info
    f.argtypes = [C.c_void_p, C.c_void_p]
    out = SagePreparedInfo()
    _chk(int(f(handle, C.byref(out))), "sage_keyframe_info")
    return out


class PreparedKeyframe:
    """``SagePreparedKeyframe``: a keyframe's pose-independent preparation (relaid planes, ordered samples, pre-sampled source
    features), made once and shared between windows (``Window(..., prepared={kf: handle})``).  Holds the caller's reference
    and keeps the device arrays the handle borrows (``dk``) alive."""

    def __init__(self, handle: int, dk: DeviceKeyframe, cfg: SageWindowConfig):
        self.h = C.c_void_p(handle)
        self.dk = dk
        self.cfg = cfg

    @classmethod
    def prepare(cls, ws: "Workspace", cfg: SageWindowConfig, dk: DeviceKeyframe) -> "PreparedKeyframe":
        """``sage_keyframe_prepare``"""
        f = lib().sage_keyframe_prepare
        f.argtypes = [C.c_void_p] * 4
        v, out = dk.view(), C.c_void_p()
        _chk(int(f(ws.h, C.byref(cfg), C.byref(v), C.byref(out))), "sage_keyframe_prepare")
        return cls(out.value, dk, cfg)

    @classmethod
    def prepare_batch(cls, ws: "Workspace", cfg: SageWindowConfig, dks) -> list:
        """``sage_keyframe_prepare_batch``: B keyframes in the launches of one"""
        dks = list(dks)
        views = (SageKeyframeView * max(1, len(dks)))(*[dk.view() for dk in dks])
        out = (C.c_void_p * max(1, len(dks)))()
        _chk(keyframe_prepare_batch_raw(ws.h, C.byref(cfg), views, len(dks), out), "sage_keyframe_prepare_batch")
        return [cls(out[b], dk, cfg) for b, dk in enumerate(dks)]

    def info(self) -> SagePreparedInfo:
        return keyframe_info_raw(self.h)

    def get(self, what: int) -> np.ndarray:
        """``sage_keyframe_get``: SAGE_PREP_PACKED [3, FS/4, P, 4] f32, _LOC [slots] i64, _HOMO [slots, 3] f32, _F0S
        [L, FS/4, slots, 4] f32"""
        i, FS, L, P = self.info(), self.cfg.FS, self.cfg.pyr.levels, self.cfg.pyr.P
        shape, dtype = {SAGE_PREP_PACKED: ((3, FS // 4, P, 4), np.float32), SAGE_PREP_LOC: ((i.slots,), np.int64),
                        SAGE_PREP_HOMO: ((i.slots, 3), np.float32), SAGE_PREP_F0S: ((L, FS // 4, i.slots, 4), np.float32)}[what]
        a = np.zeros(shape, dtype=dtype)
        f = lib().sage_keyframe_get
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        _chk(int(f(self.h, int(what), a.ctypes.data, a.nbytes)), "sage_keyframe_get")
        return a

    def release(self):
        """drops the caller's reference (``sage_keyframe_release``); windows that hold the handle keep it alive"""
        if self.h:
            lib().sage_keyframe_release(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


SAGE_PRIOR_MAX_KEYFRAMES = 16


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def schur_marginal_raw(A_ptr, g_ptr, e, n, drop_ptr, n_drop, Lambda_ptr, eta_ptr, c_ptr) -> int:
    """``sage_schur_marginal`` with raw addresses (None -> NULL) -> status code"""
    f = lib().sage_schur_marginal
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(A_ptr, g_ptr, float(e), int(n), drop_ptr, int(n_drop), Lambda_ptr, eta_ptr, c_ptr))


def schur_marginal(A, g, e: float, drop, check=True):
    """``sage_schur_marginal``: the system (A [n,n], g [n], e) with the rows ``drop`` eliminated -> (Lambda, eta, c) over the
    other rows, ascending; with ``check=False`` the status code comes first and nothing is raised."""
    A = _f64(A); g = _f64(g)
    n = g.size
    d = np.ascontiguousarray(drop, np.int32).reshape(-1)
    nk = max(n - d.size, 0)
    Lam = np.full((nk, nk), np.nan); eta = np.full(nk, np.nan); c = C.c_double(float("nan"))
    rc = schur_marginal_raw(A.ctypes.data, g.ctypes.data, e, n, d.ctypes.data if d.size else None, d.size, Lam.ctypes.data,
                            eta.ctypes.data, C.addressof(c))
    if not check:
        return rc, Lam, eta, c.value
    _chk(rc, "sage_schur_marginal")
    return Lam, eta, c.value


def marginal_prior_create_raw(m, CS, Lambda_ptr, eta_ptr, c, pose_ptr, code_ptr, scale_ptr, ids_ptr, out_ptr) -> int:
    """``sage_marginal_prior_create`` with raw addresses (None -> NULL) -> status code"""
    f = lib().sage_marginal_prior_create
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 5
    return int(f(int(m), int(CS), Lambda_ptr, eta_ptr, float(c), pose_ptr, code_ptr, scale_ptr, ids_ptr, out_ptr))


class MarginalPrior:
    """``SageMarginalPrior``: Lambda [mB,mB], eta [mB], c over m keyframes, linearised at (pose12 [m,12], code [m,CS],
    scale [m]); ``keyframes``: the ids they had in the window the prior came from."""

    def __init__(self, Lambda=None, eta=None, c=0.0, pose12=None, code=None, scale=None, keyframes=None, handle=None):
        L = lib()
        L.sage_marginal_prior_destroy.restype = None
        L.sage_marginal_prior_destroy.argtypes = [C.c_void_p]
        if handle is not None:
            self.h = C.c_void_p(handle)
        else:
            pose = _f32(pose12).reshape(-1, 12); code = _f32(code).reshape(pose.shape[0], -1); scale = _f32(scale).reshape(-1)
            m, CS = pose.shape[0], code.shape[1]
            Lam = _f64(Lambda); eta_ = _f64(eta)
            assert Lam.shape == (m * (7 + CS),) * 2 and eta_.shape == (m * (7 + CS),) and scale.size == m
            ids = np.ascontiguousarray(keyframes if keyframes is not None else np.arange(m), np.int32)
            assert ids.size == m
            self.h = C.c_void_p()
            _chk(marginal_prior_create_raw(m, CS, Lam.ctypes.data, eta_.ctypes.data, c, pose.ctypes.data, code.ctypes.data,
                                           scale.ctypes.data, ids.ctypes.data, C.addressof(self.h)), "sage_marginal_prior_create")
        m, CS = C.c_int(), C.c_int()
        f = L.sage_marginal_prior_dims
        f.argtypes = [C.c_void_p] * 3
        _chk(int(f(self.h, C.addressof(m), C.addressof(CS))), "sage_marginal_prior_dims")
        self.m, self.CS = m.value, CS.value
        self.B = 7 + self.CS

    def get(self) -> dict:
        """host copies: Lambda, eta, c, pose12, code, scale, keyframes"""
        n = self.m * self.B
        Lam = np.zeros((n, n)); eta = np.zeros(n); c = C.c_double()
        pose = np.zeros((self.m, 12), np.float32); code = np.zeros((self.m, self.CS), np.float32)
        scale = np.zeros(self.m, np.float32); ids = np.zeros(self.m, np.int32)
        f = lib().sage_marginal_prior_get
        f.argtypes = [C.c_void_p] * 7
        _chk(int(f(self.h, Lam.ctypes.data, eta.ctypes.data, C.addressof(c), pose.ctypes.data, code.ctypes.data,
                   scale.ctypes.data)), "sage_marginal_prior_get")
        g = lib().sage_marginal_prior_keyframes
        g.argtypes = [C.c_void_p] * 2
        _chk(int(g(self.h, ids.ctypes.data)), "sage_marginal_prior_keyframes")
        return dict(Lambda=Lam, eta=eta, c=c.value, pose12=pose, code=code, scale=scale, keyframes=ids)

    def evaluate(self, pose12, code, scale) -> dict:
        """``sage_prior_evaluate`` at the variables of the prior's m keyframes -> dict(delta, Atb, err)"""
        return prior_evaluate(self, pose12, code, scale)

    def close(self):
        if getattr(self, "h", None):
            lib().sage_marginal_prior_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prior_evaluate_raw(prior_handle, pose_ptr, code_ptr, scale_ptr, delta_ptr, Atb_ptr, err_ptr) -> int:
    """``sage_prior_evaluate`` with raw addresses (None -> NULL) -> status code"""
    f = lib().sage_prior_evaluate
    f.argtypes = [C.c_void_p] * 7
    return int(f(prior_handle, pose_ptr, code_ptr, scale_ptr, delta_ptr, Atb_ptr, err_ptr))


def prior_evaluate(prior: MarginalPrior, pose12, code, scale) -> dict:
    """the host mirror of the device term: delta [mB], Atb = eta - Lambda delta, err = delta' Lambda delta - 2 eta' delta + c"""
    pose = _f32(pose12).reshape(prior.m, 12); code = _f32(code).reshape(prior.m, prior.CS); scale = _f32(scale).reshape(prior.m)
    n = prior.m * prior.B
    delta = np.zeros(n); Atb = np.zeros(n); err = C.c_double()
    _chk(prior_evaluate_raw(prior.h, pose.ctypes.data, code.ctypes.data, scale.ctypes.data, delta.ctypes.data, Atb.ctypes.data,
                            C.addressof(err)), "sage_prior_evaluate")
    return dict(delta=delta, Atb=Atb, err=err.value)


def prior_term_plan(K: int, links, kf_maps, rank: int = 0, world: int = 1, check=True):
    """``sage_prior_term_plan``: the prior terms with maps ``kf_maps`` added in order to a window of K keyframes and
    ``links`` -> dict(append: [(a, b)] the structure-only links appended, place: [(term, i, j, packed block, transposed)],
    owned: [0 / 1 per term]); with ``check=False`` the status code comes first and nothing is raised."""
    lk = np.ascontiguousarray(links, np.int32).reshape(-1, 2)
    m = np.array([len(k) for k in kf_maps], np.int32)
    maps = np.array([k for km in kf_maps for k in km], np.int32)
    append = np.zeros((max(1, int((m * (m - 1) // 2).sum())), 2), np.int32)
    place = np.zeros((max(1, int((m * (m + 1) // 2).sum())), 5), np.int32)
    owned = np.zeros(max(1, m.size), np.int32)
    na, npl = C.c_int32(), C.c_int32()
    f = lib().sage_prior_term_plan
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
    rc = int(f(int(K), lk.shape[0], lk.ctypes.data if lk.size else None, m.size, m.ctypes.data if m.size else None,
               maps.ctypes.data if maps.size else None, int(rank), int(world), append.ctypes.data, C.addressof(na),
               place.ctypes.data, C.addressof(npl), owned.ctypes.data))
    out = dict(append=[tuple(r) for r in append[:na.value].tolist()], place=[tuple(r) for r in place[:npl.value].tolist()],
               owned=owned[:m.size].tolist()) if rc == 0 else None
    if not check:
        return rc, out
    _chk(rc, "sage_prior_term_plan")
    return out


def photometric_jac_error(ws: Workspace, R10, t10, R0, t0, R1, t1, bias0, basis0, code0, mask1, loc1d, homo,
                          feat0, feat1, grad1, scale0, pyr: SagePyramid, eps, weights, FS, CS):
    """``df::photometric_jac_error_calculate<CS,FS>``; poses/code are small host arrays uploaded here (the
    reference does the same H2D copies in ``PhotometricFactor::ComputeJacobianAndError``)."""
    import torch
    D = 13 + CS
    small = torch.from_numpy(np.concatenate([_f32(x).reshape(-1) for x in (R10, t10, R0, t0, R1, t1, code0)])).cuda()
    o = [0, 9, 12, 21, 24, 33, 36]
    AtA = torch.empty((D, D), dtype=torch.float32, device="cuda")
    Atb = torch.empty((D,), dtype=torch.float32, device="cuda")
    err = C.c_float(); nin = C.c_float()
    w = _f32(weights)
    N = int(homo.shape[0])
    base = small.data_ptr()
    p = lambda i: C.c_void_p(base + 4 * o[i])
    _chk(lib().sage_photometric_jac_error_calculate(
        ws.h, dptr(AtA), dptr(Atb), C.byref(err), C.byref(nin), p(0), p(1), p(2), p(3), p(4), p(5),
        dptr(bias0), dptr(basis0), p(6), dptr(mask1), dptr(loc1d), dptr(homo), dptr(feat0), dptr(feat1),
        dptr(grad1), C.c_float(scale0), C.byref(pyr), C.c_float(eps), _fp(w), N, FS, CS),
        "sage_photometric_jac_error_calculate")
    return dict(AtA=AtA.cpu().numpy(), Atb=Atb.cpu().numpy(), error=err.value, num_inliers=nin.value)


def photometric_error(ws: Workspace, R10, t10, bias0, basis0, code0, mask1, loc1d, homo, feat0, feat1, scale0,
                      pyr: SagePyramid, eps, weights, FS, CS):
    import torch
    small = torch.from_numpy(np.concatenate([_f32(x).reshape(-1) for x in (R10, t10, code0)])).cuda()
    base = small.data_ptr()
    err = C.c_float(); nin = C.c_float()
    w = _f32(weights)
    N = int(homo.shape[0])
    _chk(lib().sage_photometric_error_calculate(
        ws.h, C.byref(err), C.byref(nin), C.c_void_p(base), C.c_void_p(base + 36), dptr(bias0), dptr(basis0),
        C.c_void_p(base + 48), dptr(mask1), dptr(loc1d), dptr(homo), dptr(feat0), dptr(feat1), C.c_float(scale0),
        C.byref(pyr), C.c_float(eps), _fp(w), N, FS, CS), "sage_photometric_error_calculate")
    return err.value, nin.value


def tracker_photo_jac_error(ws: Workspace, dof, R, t, mask1, dpts0, homo, feat0s, feat1, grad1, pyr, scale0, eps,
                            weights_dev, FS):
    import torch
    small = torch.from_numpy(np.concatenate([_f32(R).reshape(-1), _f32(t).reshape(-1)])).cuda()
    base = small.data_ptr()
    AtA = torch.empty((dof, dof), dtype=torch.float32, device="cuda")
    Atb = torch.empty((dof,), dtype=torch.float32, device="cuda")
    err = C.c_float(); nin = C.c_float()
    N = int(homo.shape[0])
    _chk(lib().sage_tracker_photo_jac_error_calculate(
        ws.h, dof, dptr(AtA), dptr(Atb), C.byref(err), C.byref(nin), C.c_void_p(base), C.c_void_p(base + 36),
        dptr(mask1), dptr(dpts0), dptr(homo), dptr(feat0s), dptr(feat1), dptr(grad1), C.byref(pyr),
        C.c_float(scale0), C.c_float(eps), dptr(weights_dev), N, FS), "sage_tracker_photo_jac_error_calculate")
    return dict(AtA=AtA.cpu().numpy(), Atb=Atb.cpu().numpy(), error=err.value, num_inliers=nin.value)


def tracker_photo_error(ws: Workspace, R, t, mask1, dpts0, homo, feat0s, feat1, pyr, eps, weights_dev, FS):
    import torch
    small = torch.from_numpy(np.concatenate([_f32(R).reshape(-1), _f32(t).reshape(-1)])).cuda()
    base = small.data_ptr()
    err = C.c_float(); nin = C.c_float()
    N = int(homo.shape[0])
    _chk(lib().sage_tracker_photo_error_calculate(
        ws.h, C.byref(err), C.byref(nin), C.c_void_p(base), C.c_void_p(base + 36), dptr(mask1), dptr(dpts0),
        dptr(homo), dptr(feat0s), dptr(feat1), C.byref(pyr), C.c_float(eps), dptr(weights_dev), N, FS),
        "sage_tracker_photo_error_calculate")
    return err.value, nin.value


def geometric_jac_error(ws: Workspace, R10, t10, R0, t0, R1, t1, bias0, basis0, code0, dpt1, dgrad1, basis1, mask1,
                        loc1d_i32, homo, scale0, scale1, cam: SageCamera, eps, loss_param, weight, CS):
    import torch
    D = 14 + 2 * CS
    small = torch.from_numpy(np.concatenate([_f32(x).reshape(-1) for x in (R10, t10, R0, t0, R1, t1, code0)])).cuda()
    o = [0, 9, 12, 21, 24, 33, 36]
    base = small.data_ptr()
    p = lambda i: C.c_void_p(base + 4 * o[i])
    AtA = torch.empty((D, D), dtype=torch.float32, device="cuda")
    Atb = torch.empty((D,), dtype=torch.float32, device="cuda")
    err = C.c_float(); nin = C.c_float()
    N = int(homo.shape[0])
    _chk(lib().sage_geometric_jac_error_calculate(
        ws.h, dptr(AtA), dptr(Atb), C.byref(err), C.byref(nin), p(0), p(1), p(2), p(3), p(4), p(5),
        dptr(bias0), dptr(basis0), p(6), dptr(dpt1), dptr(dgrad1), dptr(basis1), dptr(mask1), dptr(loc1d_i32),
        dptr(homo), C.c_float(scale0), C.c_float(scale1), C.byref(cam), C.c_float(eps), C.c_float(loss_param),
        C.c_float(weight), N, CS), "sage_geometric_jac_error_calculate")
    return dict(AtA=AtA.cpu().numpy(), Atb=Atb.cpu().numpy(), error=err.value, num_inliers=nin.value)


def geometric_error(ws: Workspace, R10, t10, bias0, basis0, code0, dpt1, mask1, loc1d_i32, homo, scale0,
                    cam: SageCamera, eps, loss_param, weight, CS):
    import torch
    small = torch.from_numpy(np.concatenate([_f32(x).reshape(-1) for x in (R10, t10, code0)])).cuda()
    base = small.data_ptr()
    err = C.c_float(); nin = C.c_float()
    N = int(homo.shape[0])
    _chk(lib().sage_geometric_error_calculate(
        ws.h, C.byref(err), C.byref(nin), C.c_void_p(base), C.c_void_p(base + 36), dptr(bias0), dptr(basis0),
        C.c_void_p(base + 48), dptr(dpt1), dptr(mask1), dptr(loc1d_i32), dptr(homo), C.c_float(scale0),
        C.byref(cam), C.c_float(eps), C.c_float(loss_param), C.c_float(weight), N, CS),
        "sage_geometric_error_calculate")
    return err.value, nin.value


def depth_and_grad(ws: Workspace, bias, basis, code, scale, H, W, CS):
    import torch
    dpt = torch.empty((H, W), dtype=torch.float32, device="cuda")
    grad = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    code_d = _dev(code, np.float32)
    _chk(lib().sage_depth_and_grad(ws.h, dptr(dpt), dptr(grad), dptr(bias), dptr(basis), dptr(code_d),
                                   C.c_float(scale), H, W, CS), "sage_depth_and_grad")
    # the producer is ASYNCHRONOUS on the workspace's stream: its inputs must outlive the launch.  `code_d` rides on the
    # result (torch would otherwise hand its block to the next allocation of any thread while the kernel is queued --
    # found by tests/test_gpu_threads.py)
    dpt._sage_keepalive = code_d
    grad._sage_keepalive = code_d    # (a caller may keep only one of the two)
    return dpt, grad


DEPTH_VARIANCE, DEPTH_SIGMA = 0, 1


class SageDepthSigmaItem(C.Structure):
    _fields_ = [("bias_dev", C.c_void_p), ("basis_dev", C.c_void_p), ("code_dev", C.c_void_p), ("scale", C.c_float),
                ("cov_code_scale", C.c_void_p), ("out_dev", C.c_void_p)]


def depth_sigma_batch_raw(ws, items, n, H, W, CS, mode) -> int:
    """``sage_depth_sigma_batch`` with raw addresses (None -> NULL) -> status code"""
    f = lib().sage_depth_sigma_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    return int(f(ws, items, n, H, W, CS, mode))


def depth_sigma_batch(ws: Workspace, items, H, W, CS, mode=DEPTH_SIGMA, pad=0):
    """``sage_depth_sigma_batch``: ``items`` = [(bias [H*W] device, basis [H*W,CS] device, code [CS] host, scale, S [(CS+1),
    (CS+1)] host)] -> device tensor [n, H*W + pad] of depth variances / sigmas (the ``pad`` floats behind every map are
    NaN and stay NaN).  Asynchronous on the workspace's stream: the inputs ride on the result."""
    import torch
    n, HW = len(items), H * W
    out = torch.full((n, HW + pad), float("nan"), dtype=torch.float32, device="cuda")
    table = (SageDepthSigmaItem * n)()
    keep = []
    for i, (bias, basis, code, scale, S) in enumerate(items):
        code_d = _dev(code, np.float32)
        S64 = np.ascontiguousarray(S, np.float64)
        assert S64.shape == (CS + 1, CS + 1)
        keep += [bias, basis, code_d, S64]
        table[i] = SageDepthSigmaItem(bias.data_ptr(), basis.data_ptr(), code_d.data_ptr(), float(scale), S64.ctypes.data,
                                      out[i].data_ptr())
    _chk(depth_sigma_batch_raw(ws.h, C.addressof(table), n, H, W, CS, int(mode)), "sage_depth_sigma_batch")
    out._sage_keepalive = keep
    return out


def window_covariance_raw(w, damp_out) -> int:
    f = lib().sage_window_covariance
    f.argtypes = [C.c_void_p, C.c_void_p]
    return int(f(w, damp_out))


def window_get_covariance_raw(w, a, b, Sigma) -> int:
    f = lib().sage_window_get_covariance
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return int(f(w, a, b, Sigma))


def window_depth_sigma_raw(w, kfs, n, mode, out_dev) -> int:
    f = lib().sage_window_depth_sigma
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return int(f(w, kfs, n, mode, out_dev))


# --------------------------------------------------------------------------- TSDF fusion
SAGE_TSDF_MAX_VIEWS = 1024
TSDF_NO_CULL, TSDF_BRICK_X1, TSDF_BRICK_X2, TSDF_BRICK_X4 = 1, 1 << 4, 2 << 4, 3 << 4
TSDF_STD_ONE, TSDF_STD_SIGMA = 0, 1


class SageTsdfPlan(C.Structure):
    _fields_ = [("dim", C.c_int32 * 3), ("with_color", C.c_int32), ("origin", C.c_float * 3), ("voxel_size", C.c_float),
                ("trunc_margin", C.c_float), ("voxels", C.c_int64), ("device_bytes", C.c_int64)]


class SageTsdfView(C.Structure):
    _fields_ = [("depth_dev", C.c_void_p), ("std_dev", C.c_void_p), ("mask_dev", C.c_void_p), ("color_dev", C.c_void_p),
                ("image_floats", C.c_int64), ("pose12", C.c_float * 12), ("cam", SageCamera), ("obs_weight", C.c_float),
                ("min_depth", C.c_float), ("std_floor", C.c_float)]


class SageTsdfStats(C.Structure):
    _fields_ = [("bricks", C.c_int64), ("pairs", C.c_int64), ("pairs_kept", C.c_int64), ("views", C.c_int32),
                ("brick", C.c_int32 * 3)]


def _camera_struct(cam) -> SageCamera:
    return cam if isinstance(cam, SageCamera) else SageCamera(cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)


def tsdf_frustum_bounds_raw(cam_ptr, pose_ptr, max_depth, bounds_ptr) -> int:
    f = lib().sage_tsdf_frustum_bounds
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    return int(f(cam_ptr, pose_ptr, max_depth, bounds_ptr))


def tsdf_frustum_bounds(cam, pose12, max_depth, bounds=None) -> np.ndarray:
    """``sage_tsdf_frustum_bounds``: the view's frustum folded into ``bounds`` [min xyz, max xyz] (default zeros: the
    script's start, a volume that contains the world origin) -> the new bounds"""
    b = np.zeros(6, np.float64) if bounds is None else np.array(bounds, np.float64).reshape(6)
    c, p = _camera_struct(cam), _f32(pose12).reshape(12)
    _chk(tsdf_frustum_bounds_raw(C.addressof(c), p.ctypes.data, float(max_depth), b.ctypes.data), "sage_tsdf_frustum_bounds")
    return b


def tsdf_plan_raw(bounds_ptr, base_voxel, max_voxels, trunc_multiplier, with_color, out_ptr) -> int:
    f = lib().sage_tsdf_plan
    f.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
    return int(f(bounds_ptr, base_voxel, max_voxels, trunc_multiplier, with_color, out_ptr))


def tsdf_plan(bounds, base_voxel=0.1, max_voxels=64.0e6, trunc_multiplier=10.0, with_color=False) -> SageTsdfPlan:
    """``sage_tsdf_plan`` -> ``SageTsdfPlan`` (dim, origin, voxel_size, trunc_margin, voxels, device_bytes)"""
    b = np.ascontiguousarray(bounds, np.float64).reshape(6)
    out = SageTsdfPlan()
    _chk(tsdf_plan_raw(b.ctypes.data, base_voxel, max_voxels, trunc_multiplier, int(with_color), C.addressof(out)), "sage_tsdf_plan")
    return out


def tsdf_plan_exact(dim, origin, voxel_size, trunc_margin, with_color=False) -> SageTsdfPlan:
    """a plan of exactly these dimensions (tests, benchmarks): what ``sage_tsdf_plan`` would fill in"""
    p = SageTsdfPlan()
    p.dim[:] = [int(d) for d in dim]
    p.origin[:] = [float(o) for o in origin]
    p.with_color, p.voxel_size, p.trunc_margin = int(with_color), float(voxel_size), float(trunc_margin)
    p.voxels = int(np.prod([int(d) for d in dim]))
    p.device_bytes = p.voxels * 4 * (3 if with_color else 2)
    return p


def tsdf_view(depth, pose12, cam, std=None, mask=None, color=None, obs_weight=1.0, min_depth=1.0e-4, std_floor=0.0,
              image_floats=None) -> SageTsdfView:
    """a ``SageTsdfView`` of device tensors (None -> NULL); the tensors ride on the struct"""
    v = SageTsdfView()
    v.depth_dev, v.std_dev, v.mask_dev, v.color_dev = [t.data_ptr() if t is not None else None for t in (depth, std, mask, color)]
    v.image_floats = int(depth.numel() if image_floats is None else image_floats)
    v.pose12[:] = [float(x) for x in np.asarray(pose12, np.float32).reshape(12)]
    v.cam = _camera_struct(cam)
    v.obs_weight, v.min_depth, v.std_floor = float(obs_weight), float(min_depth), float(std_floor)
    v._sage_keepalive = (depth, std, mask, color)
    return v


def tsdf_integrate_raw(vol, view_ptr) -> int:
    f = lib().sage_tsdf_integrate
    f.argtypes = [C.c_void_p, C.c_void_p]
    return int(f(vol, view_ptr))


def tsdf_integrate_batch_raw(vol, views_ptr, n, flags) -> int:
    f = lib().sage_tsdf_integrate_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return int(f(vol, views_ptr, n, flags))


def tsdf_create_raw(ws, plan_ptr, out_ptr) -> int:
    f = lib().sage_tsdf_create
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(ws, plan_ptr, out_ptr))


def tsdf_integrate_batch_launches(n: int) -> int:
    return int(lib().sage_tsdf_integrate_batch_launches(int(n)))


def tsdf_view_chunk() -> int:
    return int(lib().sage_tsdf_view_chunk())


def window_depth_range_raw(w, kfs, n, dmin, dmax) -> int:
    f = lib().sage_window_depth_range
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return int(f(w, kfs, n, dmin, dmax))


def window_fuse_tsdf_raw(w, vol, kfs, n, std_mode, std_floor, obs_weight, min_depth) -> int:
    f = lib().sage_window_fuse_tsdf
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
    return int(f(w, vol, kfs, n, std_mode, std_floor, obs_weight, min_depth))


def window_depth_range(win: "Window", kfs, check=True):
    """``sage_window_depth_range`` -> (dmin, dmax); ``check=False`` -> (status code, dmin, dmax)"""
    kf = np.ascontiguousarray(kfs, np.int32).reshape(-1)
    lo, hi = C.c_float(), C.c_float()
    rc = window_depth_range_raw(win.h, kf.ctypes.data if kf.size else None, kf.size, C.addressof(lo), C.addressof(hi))
    if not check:
        return rc, lo.value, hi.value
    _chk(rc, "sage_window_depth_range")
    return lo.value, hi.value


def window_fuse_tsdf(win: "Window", vol: "TsdfVolume", kfs, std_mode=TSDF_STD_ONE, std_floor=0.0, obs_weight=1.0,
                     min_depth=1.0e-4, check=True) -> int:
    """``sage_window_fuse_tsdf``: the window's keyframes ``kfs`` into ``vol``, in the order given -> status code"""
    kf = np.ascontiguousarray(kfs, np.int32).reshape(-1)
    rc = window_fuse_tsdf_raw(win.h if win is not None else None, vol.h if vol is not None else None,
                              kf.ctypes.data if kf.size else None, kf.size, int(std_mode), std_floor, obs_weight, min_depth)
    if check:
        _chk(rc, "sage_window_fuse_tsdf")
    return rc


class TsdfVolume:
    """``SageTsdfVolume``: tsdf, weight and (optional) color volumes on a workspace's stream; close it before the workspace."""

    def __init__(self, ws: Workspace, plan: SageTsdfPlan):
        self.ws, self.plan = ws, plan
        self.dim = tuple(int(d) for d in plan.dim)
        self.h = C.c_void_p()
        _chk(tsdf_create_raw(ws.h, C.addressof(plan), C.addressof(self.h)), "sage_tsdf_create")

    def reset(self):
        f = lib().sage_tsdf_reset
        f.argtypes = [C.c_void_p]
        _chk(int(f(self.h)), "sage_tsdf_reset")

    def get(self, color=False):
        """``sage_tsdf_get`` -> (tsdf, weight) or (tsdf, weight, color), numpy [dx, dy, dz]; drains the stream"""
        f = lib().sage_tsdf_get
        f.argtypes = [C.c_void_p] * 4
        out = [np.empty(self.dim, np.float32) for _ in range(3 if color else 2)]
        _chk(int(f(self.h, *[o.ctypes.data for o in out], *([None] if not color else []))), "sage_tsdf_get")
        return tuple(out)

    def integrate(self, view: SageTsdfView, check=True) -> int:
        rc = tsdf_integrate_raw(self.h, C.addressof(view))
        if check:
            _chk(rc, "sage_tsdf_integrate")
        return rc

    def integrate_batch(self, views, flags=0, check=True) -> int:
        table = (SageTsdfView * max(len(views), 1))(*views)
        rc = tsdf_integrate_batch_raw(self.h, C.addressof(table), len(views), int(flags))
        if check:
            _chk(rc, "sage_tsdf_integrate_batch")
        return rc

    def last_stats(self) -> SageTsdfStats:
        f = lib().sage_tsdf_last_stats
        f.argtypes = [C.c_void_p, C.c_void_p]
        out = SageTsdfStats()
        _chk(int(f(self.h, C.addressof(out))), "sage_tsdf_last_stats")
        return out

    def close(self):
        if self.h:
            f = lib().sage_tsdf_destroy
            f.argtypes, f.restype = [C.c_void_p], None
            f(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gaussian_pyramid_with_grad(ws: Workspace, feat, mask, pyr: SagePyramid, FS):
    import torch
    out = torch.empty((FS, pyr.P), dtype=torch.float32, device="cuda")
    grad = torch.empty((2, FS, pyr.P), dtype=torch.float32, device="cuda")
    _chk(lib().sage_gaussian_pyramid_with_grad(ws.h, dptr(out), dptr(grad), dptr(feat), dptr(mask), C.byref(pyr), FS),
         "sage_gaussian_pyramid_with_grad")
    return out, grad


class Window:
    """``SageWindow``: batched K-keyframe BA window on one GPU (one shard of the edge set)."""

    def __init__(self, win, rank: int = 0, world: int = 1, stream=None, use_photo=True, use_geo=True,
                 code_prior_weight=1.0e-3, scale_prior_weight=1.0e4, pose_prior_weight=1.0e4, keypoint_terms=None,
                 keypoint_links=None, holds=None, graph_terms=None, prepared=None, prior_terms=None):
        """``keypoint_terms``: optional list of dicts (``synth.make_reprojection_matches`` / ``make_match_geometry_matches`` /
        ``make_loop_mg_*``, or by hand): kind ("reprojection" | "match_geometry" | "loop_mg"), edge (2 * link + direction),
        loc0 [N] int32, homo0 [N,3], matched_2d [N,2] or loc1 [N] + homo1 [N,3], loss_param, weight and, for match geometry,
        loss (a MG_LOSS name); loop_mg: homo0, homo1 and the unscaled depths u0 [N], u1 [N].
        ``keypoint_links``: optional list of (a, b), links that carry keypoint terms only (``sage_window_add_keypoint_link``);
        they are added after the window's dense links, so their ids start at ``len(win.links)`` (``self.links`` lists both;
        a ``win`` with ``links=[]`` gives a window without a dense edge).
        ``holds``: optional dict keyframe -> mask of SAGE_HOLD_* (``sage_window_hold``).
        ``graph_terms``: optional list of dicts as ``graph_term_struct`` takes them (``synth.make_pose_graph`` makes the
        reference's loop-closure graph), added with ``sage_window_add_graph_term``.
        ``prepared``: optional dict keyframe id -> ``PreparedKeyframe``: those keyframes are added by handle
        (``sage_window_add_prepared_keyframe``: the window borrows their preparation, and their device arrays), the others as views.
        ``prior_terms``: optional list of (``MarginalPrior``, kf_map) added with ``sage_window_add_prior_term`` after everything
        else; the structure-only links they append are listed behind the others in ``self.links``.
        All are added before the finalize this constructor performs."""
        import torch
        self.win = win
        self.pyr = make_pyramid(win.cams[0], win.L)
        assert self.pyr.P == win.P
        self.mask = _dev(win.mask, np.float32)
        self.prepared = dict(prepared or {})
        self.kfs = [self.prepared[k].dk if k in self.prepared else DeviceKeyframe(kf, win.H, win.W)
                    for k, kf in enumerate(win.keyframes)]
        cfg = SageWindowConfig()
        cfg.pyr = self.pyr
        cfg.FS, cfg.CS = win.FS, win.CS
        cfg.mask_dev = self.mask.data_ptr()
        for l in range(win.L):
            cfg.photo_weights[l] = float(win.photo_weights[l])
        cfg.geo_weight, cfg.geo_loss_param, cfg.eps = win.geo_weight, win.geo_loss_param, win.eps
        cfg.code_prior_weight, cfg.scale_prior_weight, cfg.pose_prior_weight = (
            code_prior_weight, scale_prior_weight, pose_prior_weight)
        cfg.use_photo, cfg.use_geo = int(use_photo), int(use_geo)
        self.cfg = cfg
        self.h = C.c_void_p()
        sp = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(0)
        L = lib()
        _chk(L.sage_window_create(C.byref(cfg), sp, C.byref(self.h)), "sage_window_create")
        for k, (kf, dk) in enumerate(zip(win.keyframes, self.kfs)):
            pose = pack_pose(kf.R, kf.t)
            code = _f32(kf.code)
            if k in self.prepared:
                r = self.add_prepared_keyframe(self.prepared[k], pose, code, kf.scale)
                if r < 0:
                    raise SageError(r, "sage_window_add_prepared_keyframe")
                continue
            v = dk.view()
            r = L.sage_window_add_keyframe(self.h, C.byref(v), _fp(pose), _fp(code), C.c_float(kf.scale))
            if r < 0:
                raise SageError(r, "sage_window_add_keyframe")
        for a, b in win.links:
            r = L.sage_window_add_link(self.h, a, b)
            if r < 0:
                raise SageError(r, "sage_window_add_link")
            gl = getattr(win, "link_geo_loss", None)     # optional per-link Cauchy parameters (mapper.cpp:367-373)
            if gl is not None and gl[r] > 0:
                _chk(L.sage_window_set_link_geo_loss(self.h, r, C.c_float(gl[r])), "sage_window_set_link_geo_loss")
        kp_links = [tuple(l) for l in (keypoint_links or [])]
        for a, b in kp_links:
            r = self.add_keypoint_link(a, b)
            if r < 0:
                raise SageError(r, "sage_window_add_keypoint_link")
        self.links = [(min(a, b), max(a, b)) for a, b in list(win.links) + kp_links]
        for kf, what in sorted((holds or {}).items()):
            _chk(self.hold(kf, what), "sage_window_hold")
        self.keypoint_terms = list(keypoint_terms or [])
        for t in self.keypoint_terms:
            r = self.add_keypoint_term(t)
            if r < 0:
                raise SageError(r, "sage_window_add_keypoint_term")
        self.graph_terms = list(graph_terms or [])
        for t in self.graph_terms:
            r = self.add_graph_term(t)
            if r < 0:
                raise SageError(r, "sage_window_add_graph_term")
        self.prior_terms = []
        for prior, kf_map in (prior_terms or []):
            r = self.add_prior_term(prior, kf_map)
            if r < 0:
                raise SageError(r, "sage_window_add_prior_term")
        _chk(L.sage_window_set_shard(self.h, rank, world), "sage_window_set_shard")
        _chk(L.sage_window_finalize(self.h), "sage_window_finalize")
        self.K = L.sage_window_num_keyframes(self.h)
        self.B = L.sage_window_block_size(self.h)
        self.Bs = L.sage_window_solver_block_size(self.h)   # rows per keyframe in the solver (sage_window_hold)
        self.nlinks = L.sage_window_num_links(self.h)
        self.packed_count = L.sage_window_packed_count(self.h)
        self.residuals_per_linearize = L.sage_window_residuals_per_linearize(self.h)
        self.bytes_per_linearize = L.sage_window_bytes_per_linearize(self.h)

    def add_prepared_keyframe(self, pk, pose12, code, scale) -> int:
        """``sage_window_add_prepared_keyframe`` -> keyframe id, or the negative status code (``pk``: a ``PreparedKeyframe``,
        or None for NULL)"""
        f = lib().sage_window_add_prepared_keyframe
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float]
        pose, code = _f32(pose12), _f32(code)
        return int(f(self.h, pk.h if pk is not None else None, pose.ctypes.data, code.ctypes.data, float(scale)))

    def build_stats(self) -> SageWindowBuildStats:
        """``sage_window_build_stats``: what stages 3-5 of the last finalize did (keyframes, prepared, repacked, ordered,
        presampled, launches)"""
        f = lib().sage_window_build_stats
        f.argtypes = [C.c_void_p, C.c_void_p]
        out = SageWindowBuildStats()
        _chk(int(f(self.h, C.byref(out))), "sage_window_build_stats")
        return out

    def add_keypoint_link(self, a, b) -> int:
        """``sage_window_add_keypoint_link`` -> link id, or the negative status code"""
        return int(lib().sage_window_add_keypoint_link(self.h, int(a), int(b)))

    def hold(self, kf, what) -> int:
        """``sage_window_hold`` -> status code"""
        return int(lib().sage_window_hold(self.h, int(kf), int(what)))

    def add_keypoint_term(self, t) -> int:
        """``sage_window_add_keypoint_term`` with the arrays of dict ``t`` uploaded for the call (the engine copies them);
        returns the term id, or the negative status code."""
        import torch
        kind = KP_KINDS.get(t["kind"], t["kind"])
        lmg = kind == SAGE_KP_LOOP_MG
        mg = "loc1" in t and not lmg
        N = int(np.asarray(t["homo0"]).shape[0])
        dev = dict(homo0=_dev(t["homo0"], np.float32))
        kt = SageKeypointTerm()
        kt.kind = int(kind)
        kt.edge, kt.N = int(t["edge"]), N
        kt.homo0 = dev["homo0"].data_ptr()
        if not lmg:
            dev["loc0"] = _dev(t["loc0"], np.int32)
            kt.loc1d_0 = dev["loc0"].data_ptr()
        if lmg:                                           # (a missing array stays NULL: the engine answers SAGE_E_INVALID)
            for key, field in (("homo1", "matched_homo1"), ("u0", "unscaled_dpts0"), ("u1", "matched_unscaled_dpts1")):
                if t.get(key) is not None:
                    dev[key] = _dev(t[key], np.float32)
                    setattr(kt, field, dev[key].data_ptr())
        elif mg:
            dev["loc1"] = _dev(t["loc1"], np.int32); dev["homo1"] = _dev(t["homo1"], np.float32)
            kt.matched_loc1d_1, kt.matched_homo1 = dev["loc1"].data_ptr(), dev["homo1"].data_ptr()
            loss = t.get("loss", "fair")
            kt.loss = MG_LOSS[loss] if isinstance(loss, str) else int(loss)
        else:
            dev["m2d"] = _dev(t["matched_2d"], np.float32)
            kt.matched_2d = dev["m2d"].data_ptr()
        kt.loss_param, kt.weight = float(t["loss_param"]), float(t["weight"])
        torch.cuda.synchronize()
        return int(lib().sage_window_add_keypoint_term(self.h, C.byref(kt)))

    def num_keypoint_terms(self) -> int:
        return int(lib().sage_window_num_keypoint_terms(self.h))

    def get_keypoint_term(self, i, check=True):
        """host copy of term i's last linearize -> dict(AtA [D,D], Atb [D], error, num_inliers); with ``check=False`` the
        status code is returned next to the dict instead of raising."""
        kind = self.keypoint_terms[i]["kind"] if 0 <= i < len(self.keypoint_terms) else "reprojection"
        D = kp_term_dim(kind, self.win.CS)
        A = np.zeros((D, D), np.float32); b = np.zeros(D, np.float32)
        err = C.c_float(); nin = C.c_float()
        rc = lib().sage_window_get_keypoint_term(self.h, int(i), _fp(A), _fp(b), C.byref(err), C.byref(nin))
        out = dict(AtA=A, Atb=b, error=err.value, num_inliers=nin.value)
        if not check:
            return rc, out
        _chk(rc, "sage_window_get_keypoint_term")
        return out

    def add_graph_term(self, t) -> int:
        """``sage_window_add_graph_term`` of dict ``t`` (``graph_term_struct``) -> term id, or the negative status code"""
        gt = graph_term_struct(t)
        return int(lib().sage_window_add_graph_term(self.h, C.byref(gt)))

    def num_graph_terms(self) -> int:
        return int(lib().sage_window_num_graph_terms(self.h))

    def get_graph_term(self, i, check=True):
        """host copy of graph term i's last linearize -> dict(AtA [14,14], Atb [14], error); with ``check=False`` the status
        code is returned next to the dict instead of raising."""
        A = np.zeros((GRAPH_TERM_DIM, GRAPH_TERM_DIM), np.float32); b = np.zeros(GRAPH_TERM_DIM, np.float32)
        err = C.c_float()
        rc = lib().sage_window_get_graph_term(self.h, int(i), _fp(A), _fp(b), C.byref(err))
        out = dict(AtA=A, Atb=b, error=err.value)
        if not check:
            return rc, out
        _chk(rc, "sage_window_get_graph_term")
        return out

    def add_prior_term(self, prior, kf_map) -> int:
        """``sage_window_add_prior_term`` -> term id, or the negative status code (``prior``: a ``MarginalPrior`` or None for
        NULL; ``kf_map``: this window's keyframes behind the prior's rows, or None).  ``self.links`` grows by the
        structure-only links the call appended."""
        f = lib().sage_window_add_prior_term
        f.argtypes = [C.c_void_p] * 3
        km = np.ascontiguousarray(kf_map, np.int32) if kf_map is not None else None
        before = lib().sage_window_num_links(self.h)
        r = int(f(self.h, prior.h if prior is not None else None, km.ctypes.data if km is not None else None))
        if r >= 0:
            from itertools import combinations
            have = set(self.links)
            new = sorted({(min(a, b), max(a, b)) for a, b in combinations(km.tolist(), 2)} - have)
            assert lib().sage_window_num_links(self.h) - before == len(new)
            self.links = self.links + new
            self.prior_terms.append((prior, km.tolist()))
        return r

    def num_prior_terms(self) -> int:
        return int(lib().sage_window_num_prior_terms(self.h))

    def get_prior_term(self, i, check=True):
        """host copy of prior term i's last linearize in doubles -> dict(AtA [mB,mB], Atb [mB], err); with ``check=False``
        the status code is returned next to the dict instead of raising."""
        m = self.prior_terms[i][0].m if 0 <= i < len(self.prior_terms) else 1
        n = m * (7 + self.win.CS)
        A = np.zeros((n, n)); b = np.zeros(n); err = C.c_double()
        f = lib().sage_window_get_prior_term
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = int(f(self.h, int(i), A.ctypes.data, b.ctypes.data, C.addressof(err)))
        out = dict(AtA=A, Atb=b, err=err.value)
        if not check:
            return rc, out
        _chk(rc, "sage_window_get_prior_term")
        return out

    def marginalize(self, drop, check=True):
        """``sage_window_marginalize``: the ``MarginalPrior`` the keyframes ``drop`` leave behind; with ``check=False`` ->
        (status code, prior or None)."""
        d = np.ascontiguousarray(drop, np.int32).reshape(-1)
        h = C.c_void_p()
        f = lib().sage_window_marginalize
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        rc = int(f(self.h, d.ctypes.data if d.size else None, d.size, C.addressof(h)))
        prior = MarginalPrior(handle=h.value) if rc == 0 else None
        if not check:
            return rc, prior
        _chk(rc, "sage_window_marginalize")
        return prior

    def covariance(self, check=True):
        """``sage_window_covariance``: the marginal covariances of the last solve -> that solve's damping; with
        ``check=False`` -> (status code, damping)."""
        damp = C.c_double(-1.0)
        rc = window_covariance_raw(self.h, C.addressof(damp))
        if not check:
            return rc, damp.value
        _chk(rc, "sage_window_covariance")
        return damp.value

    def get_covariance(self, a, b, check=True):
        """``sage_window_get_covariance``: block (a, b) of the stored Sigma [B, B] (a == b, or a link either way round); with
        ``check=False`` -> (status code, block)."""
        S = np.zeros((self.B, self.B), np.float64)
        rc = window_get_covariance_raw(self.h, int(a), int(b), S.ctypes.data)
        if not check:
            return rc, S
        _chk(rc, "sage_window_get_covariance")
        return S

    def depth_sigma(self, kfs, mode=DEPTH_SIGMA, check=True):
        """``sage_window_depth_sigma``: the depth variance / sigma maps of the keyframes ``kfs`` under the stored Sigma -> device
        tensor [n, H, W] (the launch is enqueued on the window's stream; ``.cpu()`` of the result waits for it only on the
        default stream: synchronise first when the window has a stream of its own); ``check=False`` -> (status code, tensor)."""
        import torch
        kf = np.ascontiguousarray(kfs, np.int32).reshape(-1)
        out = torch.zeros((kf.size, self.win.H, self.win.W), dtype=torch.float32, device="cuda")
        ptrs = (C.c_void_p * max(kf.size, 1))(*[out[i].data_ptr() for i in range(kf.size)])
        rc = window_depth_sigma_raw(self.h, kf.ctypes.data if kf.size else None, kf.size, int(mode), ptrs)
        if not check:
            return rc, out
        _chk(rc, "sage_window_depth_sigma")
        return out

    def depth_sigma_timing(self, reps, mode=DEPTH_SIGMA):
        """``sage_window_depth_sigma_timing`` -> (median us of the sigma kernel over all keyframes, of depth_batch_kernel)"""
        f = lib().sage_window_depth_sigma_timing
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        a, b = C.c_double(), C.c_double()
        _chk(int(f(self.h, int(mode), int(reps), C.addressof(a), C.addressof(b))), "sage_window_depth_sigma_timing")
        return a.value, b.value

    # raw-pointer views for torch.distributed (plumbing only)
    def packed_tensor(self):
        return _tensor_from_ptr(lib().sage_window_packed_dev(self.h), self.packed_count)

    def error_tensor(self):
        return _tensor_from_ptr(lib().sage_window_error_dev(self.h), 4)

    def linearize(self):
        _chk(lib().sage_window_linearize(self.h), "sage_window_linearize")

    def error(self, which=1):
        _chk(lib().sage_window_error(self.h, which), "sage_window_error")

    def tune_runs(self):
        """``sage_window_tune_runs``: measure the photometric kernels' run lengths on this window, keep the fastest ->
        dict(tpb, tpb_rule, ms_rule, ms_best)."""
        tpb, rule = C.c_int(0), C.c_int(0)
        ms_rule, ms_best = C.c_float(0), C.c_float(0)
        _chk(lib().sage_window_tune_runs(self.h, C.byref(tpb), C.byref(rule), C.byref(ms_rule), C.byref(ms_best)),
             "sage_window_tune_runs")
        return dict(tpb=tpb.value, tpb_rule=rule.value, ms_rule=ms_rule.value, ms_best=ms_best.value)

    def set_runs(self, tpb):
        _chk(lib().sage_window_set_runs(self.h, int(tpb)), "sage_window_set_runs")

    def solve(self, damp, want_norm=True):
        """Damped step + candidate variables.  With ``want_norm=False`` the device solver is only enqueued (no
        synchronisation); a non-positive pivot is then reported by the next ``total_error``/``accept``."""
        if not want_norm:
            _chk(lib().sage_window_solve(self.h, C.c_double(damp), None), "sage_window_solve")
            return None
        sn = C.c_double()
        _chk(lib().sage_window_solve(self.h, C.c_double(damp), C.byref(sn)), "sage_window_solve")
        return sn.value

    def total_error(self, from_linearize: bool):
        e = C.c_double()
        _chk(lib().sage_window_total_error(self.h, int(from_linearize), C.byref(e)), "sage_window_total_error")
        return e.value

    def accept(self):
        _chk(lib().sage_window_accept(self.h), "sage_window_accept")

    def reset(self):
        _chk(lib().sage_window_reset(self.h), "sage_window_reset")

    def set_allreduce(self, dist_module, group=None):
        """Install ``torch.distributed.all_reduce`` as the window's all-reduce hook (``sage_window_set_allreduce``):
        ``lm_step`` then drives a sharded window too, entering Python only for the two collectives."""
        tensors = {}
        for t in (self.packed_tensor(), self.error_tensor()):
            tensors[(t.data_ptr(), t.numel())] = t

        def hook(ptr, n, _user):
            try:
                t = tensors.get((ptr, n))
                if t is None:
                    t = tensors[(ptr, n)] = _tensor_from_ptr(ptr, n)
                dist_module.all_reduce(t, group=group)
                return 0
            except Exception:                      # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1

        self._allreduce_cb = ALLREDUCE_FN(hook)    # keep the trampoline alive as long as the window
        _chk(lib().sage_window_set_allreduce(self.h, self._allreduce_cb, None), "sage_window_set_allreduce")

    def sync_variables(self):
        _chk(lib().sage_window_sync_variables(self.h), "sage_window_sync_variables")

    def use_rccl(self, comm):
        """native RCCL all-reduce on the window's stream (sage_window_use_rccl); comm from rccl_comm_create()."""
        _chk(lib().sage_window_use_rccl(self.h, C.c_void_p(comm)), "sage_window_use_rccl")

    def emulate_peers(self, rest):
        """``sage_window_emulate_peers``: rest = [n_iterates, packed_count] float64 cuda tensor (kept alive here), the
        packed systems of the ranks that are not there at the LM iterates since reset; None switches it off."""
        if rest is None:
            self._emu_rest = None
            _chk(lib().sage_window_emulate_peers(self.h, None, 0), "sage_window_emulate_peers")
            return
        assert rest.is_cuda and rest.dim() == 2 and rest.shape[1] == self.packed_count and rest.is_contiguous()
        self._emu_rest = rest
        _chk(lib().sage_window_emulate_peers(self.h, C.c_void_p(rest.data_ptr()), int(rest.shape[0])),
             "sage_window_emulate_peers")

    def lm_step(self, state: SageLmState, cfg: SageLmConfig):
        _chk(lib().sage_window_lm_step(self.h, C.byref(state), C.byref(cfg)), "sage_window_lm_step")
        return state

    def lm_run(self, state: SageLmState, cfg: SageLmConfig, n: int):
        """n LM iterations without returning to Python in between -> [n, 4] trace {error, candidate, accepted, damp}."""
        tr = np.zeros((n, 4), np.float64)
        done = C.c_int()
        _chk(lib().sage_window_lm_run(self.h, C.byref(state), C.byref(cfg), n, tr.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(done)), "sage_window_lm_run")
        return tr[:done.value]

    def lm_run_timed(self, state: SageLmState, cfg: SageLmConfig, n: int):
        """lm_run + the host wall time of every iteration in seconds -> ([n, 4] trace, [n] seconds)."""
        tr = np.zeros((n, 4), np.float64); sec = np.zeros(n, np.float64)
        done = C.c_int()
        _chk(lib().sage_window_lm_run_timed(self.h, C.byref(state), C.byref(cfg), n, tr.ctypes.data_as(C.POINTER(C.c_double)),
                                            C.byref(done), sec.ctypes.data_as(C.POINTER(C.c_double))), "sage_window_lm_run_timed")
        return tr[:done.value], sec[:done.value]

    def dogleg_step(self, state: SageDoglegState, cfg: SageDoglegConfig):
        """one dogleg iteration (``sage_window_dogleg_step``): linearize, one solve at damping 0, the products, the
        trust-region policy around candidate + error pass, accept or keep"""
        _chk(lib().sage_window_dogleg_step(self.h, C.byref(state), C.byref(cfg)), "sage_window_dogleg_step")
        return state

    def dogleg_run(self, state: SageDoglegState, cfg: SageDoglegConfig, n: int):
        """n dogleg iterations without returning to Python in between -> [n, 7] trace {error, candidate, accepted, delta
        after the step, rho, region, evals}."""
        tr = np.zeros((n, 7), np.float64)
        done = C.c_int()
        _chk(lib().sage_window_dogleg_run(self.h, C.byref(state), C.byref(cfg), n, tr.ctypes.data_as(C.POINTER(C.c_double)),
                                          C.byref(done)), "sage_window_dogleg_run")
        return tr[:done.value]

    def dogleg_products(self):
        """``sage_window_dogleg_products`` (after ``linearize`` and ``solve(0)``) -> dots [6] in the order of DOGLEG_DOTS"""
        d = np.zeros(6, np.float64)
        _chk(lib().sage_window_dogleg_products(self.h, d.ctypes.data_as(C.POINTER(C.c_double))), "sage_window_dogleg_products")
        return d

    def dogleg_candidate(self, a, b):
        """``sage_window_dogleg_candidate``: the candidate for delta = a g + b n (after ``dogleg_products``)"""
        f = lib().sage_window_dogleg_candidate
        f.argtypes = [C.c_void_p, C.c_double, C.c_double]
        _chk(f(self.h, float(a), float(b)), "sage_window_dogleg_candidate")

    def dogleg_vectors(self):
        """host copies of (g, Ag, n, An), K * B doubles each (``sage_window_get_dogleg_vectors``)"""
        v = [np.zeros(self.K * self.B, np.float64) for _ in range(4)]
        _chk(lib().sage_window_get_dogleg_vectors(self.h, *[x.ctypes.data_as(C.POINTER(C.c_double)) for x in v]),
             "sage_window_get_dogleg_vectors")
        return tuple(v)

    def set_relinearization(self, mode: int, check=True) -> int:
        """``sage_window_set_relinearization`` (SAGE_RELIN_ALL / SAGE_RELIN_STALE); ``check=False``: the status code"""
        rc = int(lib().sage_window_set_relinearization(self.h, int(mode)))
        if check:
            _chk(rc, "sage_window_set_relinearization")
        return rc

    def last_evaluation(self) -> dict:
        """``sage_window_last_evaluation`` -> the ``SageEvalCounts`` of the last linearize as a dict"""
        n = SageEvalCounts()
        _chk(lib().sage_window_last_evaluation(self.h, C.byref(n)), "sage_window_last_evaluation")
        return n.as_dict()

    def relin_marks(self, t: SageRelinThresholds):
        """``sage_window_relin_marks`` on the last solve's delta -> (marks [K] int32, groups marked)"""
        marks = np.zeros(self.K, np.int32); n = C.c_int32()
        _chk(lib().sage_window_relin_marks(self.h, C.byref(t), marks.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n)),
             "sage_window_relin_marks")
        return marks, n.value

    def accept_marked(self, marks):
        """``sage_window_accept_marked``: candidate -> current for the marked groups only"""
        m = np.ascontiguousarray(marks, np.int32)
        assert m.size == self.K
        _chk(lib().sage_window_accept_marked(self.h, m.ctypes.data_as(C.POINTER(C.c_int32))), "sage_window_accept_marked")

    def delta(self):
        d = np.zeros(self.K * self.B, np.float64)
        _chk(lib().sage_window_get_delta(self.h, d.ctypes.data_as(C.POINTER(C.c_double))), "sage_window_get_delta")
        return d

    def get_keyframe(self, k):
        pose = np.zeros(12, np.float32); code = np.zeros(self.win.CS, np.float32); s = C.c_float()
        _chk(lib().sage_window_get_keyframe(self.h, k, _fp(pose), _fp(code), C.byref(s)), "sage_window_get_keyframe")
        return pose, code, s.value

    def set_keyframe(self, k, pose12, code, scale):
        pose12 = _f32(pose12); code = _f32(code)
        _chk(lib().sage_window_set_keyframe(self.h, k, _fp(pose12), _fp(code), C.c_float(scale)),
             "sage_window_set_keyframe")

    def get_edge(self, type_, e):
        D = 13 + self.win.CS if type_ == 0 else 14 + 2 * self.win.CS
        A = np.zeros((D, D), np.float32); b = np.zeros(D, np.float32)
        err = C.c_float(); nin = C.c_float()
        _chk(lib().sage_window_get_edge(self.h, type_, e, _fp(A), _fp(b), C.byref(err), C.byref(nin)),
             "sage_window_get_edge")
        return dict(AtA=A, Atb=b, error=err.value, num_inliers=nin.value)

    def prepass(self, poses12, codes, scales, jacobians: bool = True) -> bool:
        """f2: evaluate the whole window once at these values (or hit the cache). Returns True when kernels ran."""
        P = _f32(np.asarray(poses12).reshape(-1)); Cd = _f32(np.asarray(codes).reshape(-1)); S = _f32(np.asarray(scales).reshape(-1))
        K = self.K
        assert P.size == K * 12 and Cd.size == K * self.win.CS and S.size == K
        rec = C.c_int32()
        _chk(lib().sage_window_prepass(self.h, _fp(P), _fp(Cd), _fp(S), int(jacobians), C.byref(rec)), "sage_window_prepass")
        return bool(rec.value)

    # by the number of ids in front (1: a term, 2: a dense factor's type and edge): window, ids, [psd_mode,] output pointers
    _FACTOR_ARGTYPES = {n: [C.c_void_p] + [C.c_int] * (n + 1) + [C.c_void_p] * 5 for n in (1, 2)}
    _ERROR_ARGTYPES = {n: [C.c_void_p] + [C.c_int] * n + [C.c_void_p] for n in (1, 2)}

    def _cached_factor(self, name, ids, psd_mode, check):
        """one factor of the prepass cache through the C call ``name(window, *ids, psd_mode, G, g, f, dims, nkeys)`` ->
        (blocks, gs, f, dims); with ``check=False`` (status code, that tuple or None) instead of raising."""
        f_ = getattr(lib(), name)
        f_.argtypes = self._FACTOR_ARGTYPES[len(ids)]
        D = 14 + 2 * self.win.CS                                    # the widest factor
        G = np.zeros(D * (D + 1) // 2 + D * D, np.float64); g = np.zeros(D, np.float64); f = C.c_double()
        dims = (C.c_int32 * 6)(); nk = C.c_int32()
        rc = int(f_(self.h, *ids, int(psd_mode), G.ctypes.data, g.ctypes.data, C.addressof(f), C.addressof(dims), C.addressof(nk)))
        if rc != 0:
            if check:
                raise SageError(rc, name)
            return rc, None
        dims = [int(dims[k]) for k in range(nk.value)]
        blocks, gs = _blocks_of(G, g[:sum(dims)].copy(), dims)
        out = (blocks, gs, f.value, dims)
        return out if check else (rc, out)

    def _cached_error(self, name, ids, check):
        """one factor's error through ``name(window, *ids, err)`` -> the error; ``check=False``: (status code, error)"""
        f_ = getattr(lib(), name)
        f_.argtypes = self._ERROR_ARGTYPES[len(ids)]
        v = C.c_double()
        rc = int(f_(self.h, *ids, C.addressof(v)))
        if check:
            _chk(rc, name)
            return v.value
        return rc, v.value

    def factor(self, type_, e, psd_mode: int = 1):
        """f2: the HessianFactor of directed edge e from the prepass cache -> (blocks, gs, f, dims)."""
        return self._cached_factor("sage_window_factor", (int(type_), int(e)), psd_mode, True)

    def prepare_factors(self, psd_mode: int = 1, n_threads: int = 0):
        """f2: NearestPsd of every cached factor on host threads; factor(.., psd_mode) then only cuts blocks."""
        _chk(lib().sage_window_prepare_factors(self.h, psd_mode, n_threads), "sage_window_prepare_factors")

    def prepare_factors_device(self) -> "SagePsdStats":
        """f2: NearestPsd (psd_mode 1) of every cached factor on the device -- one launch per factor type, one wait;
        factor(.., 1) then only cuts blocks -> the worst ``SagePsdStats`` record."""
        worst = SagePsdStats()
        _chk(lib().sage_window_prepare_factors_device(self.h, C.byref(worst)), "sage_window_prepare_factors_device")
        return worst

    def prepare_factors_device_launches(self) -> int:
        """kernels the last ``prepare_factors_device`` launched (0: mode 1 was prepared already)"""
        f = lib().sage_window_prepare_factors_device_launches
        f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def keypoint_factor(self, i, psd_mode: int = 1, check=True):
        """f2: the HessianFactor of keypoint term i from the prepass cache -> (blocks, gs, f, dims); with ``check=False``
        (status code, that tuple or None) instead of raising."""
        return self._cached_factor("sage_window_keypoint_factor", (int(i),), psd_mode, check)

    def graph_factor(self, i, psd_mode: int = 1, check=True):
        """f2: the HessianFactor of graph term i from the prepass cache -> (blocks, gs, f, dims); ``check`` as above."""
        return self._cached_factor("sage_window_graph_factor", (int(i),), psd_mode, check)

    def keypoint_factor_error(self, i, check=True) -> float:
        return self._cached_error("sage_window_keypoint_factor_error", (int(i),), check)

    def graph_factor_error(self, i, check=True) -> float:
        return self._cached_error("sage_window_graph_factor_error", (int(i),), check)

    def factor_error(self, type_, e) -> float:
        return self._cached_error("sage_window_factor_error", (int(type_), int(e)), True)

    def set_profiling(self, on):
        """False / 0 off, True / 1 every hot kernel + phase marks, 2 the photometric linearize only."""
        _chk(lib().sage_window_set_profiling(self.h, int(on)), "sage_window_set_profiling")

    def kernel_time(self, which: int):
        """(total_ms, launches) of hot kernel `which` since the last call (0 photo lin, 1 geo lin, 2 photo err, 3 geo err,
        4 keypoint-term linearize, 5 keypoint-term error, 6 graph-term linearize, 7 graph-term error, 8 prior_eval_kernel,
        9 prior_add_kernel)."""
        ms = C.c_double(); n = C.c_int()
        _chk(lib().sage_window_get_kernel_time(self.h, which, C.byref(ms), C.byref(n)), "sage_window_get_kernel_time")
        return ms.value, n.value

    def phase_time(self):
        """({linearize, allreduce, solve, error_pass} total ms, iterations) of the LM iterations since the last call."""
        ms = (C.c_double * 4)(); n = C.c_int()
        _chk(lib().sage_window_get_phase_time(self.h, ms, C.byref(n)), "sage_window_get_phase_time")
        return dict(zip(("linearize", "allreduce", "solve", "error_pass"), (float(v) for v in ms))), n.value

    def packed_host(self):
        return self.packed_tensor().cpu().numpy()

    def close(self):
        if self.h:
            lib().sage_window_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _tensor_from_ptr(ptr: int, n: int):
    """wrap engine-owned device memory as a torch tensor (zero-copy) so torch.distributed can all-reduce it."""
    import torch

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = dict(shape=(int(n),), typestr="<f8", data=(int(ptr), False), version=2)
    return torch.as_tensor(h, device="cuda")


# --------------------------------------------------------------------------- host-side window algebra
# (pure numpy; used by the multi-process CPU tests of the sharded reduction and by parity tests)
class ShardPlan:
    """sage_shard_* : domain-decomposed solve of a link-sharded window (host, double)."""

    def __init__(self, K, links, B, rank, world):
        L = lib()
        L.sage_shard_sep_count.restype = C.c_size_t
        L.sage_shard_sep_count.argtypes = [C.c_void_p]
        lk = np.ascontiguousarray(np.asarray(links, np.int32).reshape(-1))
        self.h = C.c_void_p()
        _chk(L.sage_shard_plan_create(K, len(links), lk.ctypes.data_as(C.POINTER(C.c_int32)), B, rank, world,
                                      C.byref(self.h)), "sage_shard_plan_create")
        self.K, self.B = K, B
        self.sep_count = int(L.sage_shard_sep_count(self.h))
        self.n_sep = L.sage_shard_num_separators(self.h)
        self.n_interior = L.sage_shard_num_interior(self.h)

    def owner(self, kf):
        return lib().sage_shard_keyframe_owner(self.h, kf)

    def is_local(self, kf):
        return bool(lib().sage_shard_keyframe_is_local(self.h, kf))

    def eliminate(self, packed_local, damp, diag_add=None, g_add=None):
        p = np.ascontiguousarray(packed_local, np.float64)
        out = np.zeros(self.sep_count, np.float64)
        dp = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
        self._keep = (diag_add, g_add)
        _chk(lib().sage_shard_eliminate(self.h, p.ctypes.data_as(C.POINTER(C.c_double)), C.c_double(damp), dp(diag_add),
                                        dp(g_add), out.ctypes.data_as(C.POINTER(C.c_double))), "sage_shard_eliminate")
        return out

    def solve(self, sep_reduced):
        s = np.ascontiguousarray(sep_reduced, np.float64)
        delta = np.zeros(self.K * self.B, np.float64)
        _chk(lib().sage_shard_solve(self.h, s.ctypes.data_as(C.POINTER(C.c_double)),
                                    delta.ctypes.data_as(C.POINTER(C.c_double))), "sage_shard_solve")
        return delta

    def close(self):
        if self.h:
            lib().sage_shard_plan_destroy(self.h)
            self.h = C.c_void_p()


def rccl_unique_id() -> bytes:
    buf = (C.c_ubyte * 128)()
    _chk(lib().sage_rccl_unique_id(buf), "sage_rccl_unique_id")
    return bytes(buf)


def rccl_comm_create(uid: bytes, rank: int, world: int) -> int:
    """ncclCommInitRank on the current device -> opaque communicator handle (int)."""
    buf = (C.c_ubyte * 128).from_buffer_copy(uid)
    comm = C.c_void_p()
    _chk(lib().sage_rccl_comm_create(buf, rank, world, C.byref(comm)), "sage_rccl_comm_create")
    return comm.value


def rccl_comm_destroy(comm: int):
    lib().sage_rccl_comm_destroy(C.c_void_p(comm))


def rccl_comm_info(comm: int):
    """(ranks, rank) as the communicator itself reports them (``ncclCommCount`` / ``ncclCommUserRank``)."""
    n, r = C.c_int(), C.c_int()
    _chk(lib().sage_rccl_comm_info(C.c_void_p(comm), C.byref(n), C.byref(r)), "sage_rccl_comm_info")
    return n.value, r.value


def shard_links(nlinks: int, rank: int, world: int) -> List[int]:
    """link ownership rule of windows that use the domain-decomposed solve (``SAGE_SHARD_SCHUR`` / K >= 256) and of
    ``sage_shard_plan_create``: rank r owns the contiguous range [r*n/world, (r+1)*n/world) of the link list."""
    return list(range(nlinks * rank // world, nlinks * (rank + 1) // world))


def shard_edges(nlinks: int, rank: int, world: int) -> List[int]:
    """ownership rule of ``sage_window_set_shard`` (r05): rank r owns the contiguous range [r*2n/world, (r+1)*2n/world) of
    the DIRECTED edges 2*link + direction (both factor types of a direction together); the two directions of a link may
    belong to two ranks."""
    return list(range(2 * nlinks * rank // world, 2 * nlinks * (rank + 1) // world))


def edge_col(type_: int, role: int, bi: int, CS: int) -> int:
    """B-index (pose 6, code CS, scale) -> column of the per-edge system (mirror of the assemble kernel).  type 0: the
    photometric edge's layout (and the reprojection term's), 1: the geometric edge's (match-geometry term's), 2: the loop-MG
    term's D = 14 [pose0 pose1 scale0 scale1] -- code rows absent."""
    if bi < 6:
        return role * 6 + bi
    if type_ == 2:
        return 12 + role if bi == 6 + CS else -1
    if type_ == 0:
        if role == 1:
            return -1
        return 12 + (bi - 6) if bi < 6 + CS else 12 + CS
    if bi < 6 + CS:
        return 12 + role * CS + (bi - 6)
    return 12 + 2 * CS + role


def assemble_packed(K: int, links: Sequence, CS: int, edge_results: dict) -> np.ndarray:
    """Sum per-edge normal equations into the packed block layout.
    ``edge_results[(type, link, dir)] = dict(AtA, Atb, error, num_inliers)`` for the edges present; type as ``edge_col``
    takes it (2: a loop-MG term's 14 x 14 result; its error and count go to the geometric slots of the tail)."""
    B = 7 + CS
    BB = B * B
    diag = np.zeros((K, B, B), np.float64)
    lnk = np.zeros((len(links), B, B), np.float64)
    g = np.zeros((K, B), np.float64)
    tail = np.zeros(4, np.float64)
    cols = {(t, r): np.array([edge_col(t, r, bi, CS) for bi in range(B)]) for t in (0, 1, 2) for r in (0, 1)}
    for (t, l, d), res in edge_results.items():
        a, b = links[l]
        k0, k1 = (a, b) if d == 0 else (b, a)
        A = np.asarray(res["AtA"], np.float64); v = np.asarray(res["Atb"], np.float64)
        for kf, role in ((k0, 0), (k1, 1)):
            c = cols[(t, role)]
            m = c >= 0
            diag[kf][np.ix_(m, m)] += A[np.ix_(c[m], c[m])]
            g[kf][m] += v[c[m]]
        # link block rows = older keyframe a, cols = newer keyframe b
        ra, rb = (0, 1) if d == 0 else (1, 0)
        ca, cb = cols[(t, ra)], cols[(t, rb)]
        ma, mb = ca >= 0, cb >= 0
        lnk[l][np.ix_(ma, mb)] += A[np.ix_(ca[ma], cb[mb])]
        tail[min(t, 1)] += res["error"]
        tail[2 + min(t, 1)] += res["num_inliers"]
    return np.concatenate([diag.reshape(-1), lnk.reshape(-1), g.reshape(-1), tail])


def unpack_dense(packed: np.ndarray, K: int, links: Sequence, CS: int):
    """packed block layout -> dense (K*B x K*B) H, g, tail."""
    B = 7 + CS
    BB = B * B
    n = K * B
    H = np.zeros((n, n), np.float64)
    diag = packed[:K * BB].reshape(K, B, B)
    lnk = packed[K * BB:(K + len(links)) * BB].reshape(len(links), B, B)
    g = packed[(K + len(links)) * BB:(K + len(links)) * BB + n].astype(np.float64)
    for k in range(K):
        H[k * B:(k + 1) * B, k * B:(k + 1) * B] = 0.5 * (diag[k] + diag[k].T)
    for l, (a, b) in enumerate(links):
        H[a * B:(a + 1) * B, b * B:(b + 1) * B] += lnk[l]
        H[b * B:(b + 1) * B, a * B:(a + 1) * B] += lnk[l].T
    return H, g, packed[-4:]


def shuffle_indices(n: int, seed: int) -> np.ndarray:
    """Host helper: the keyframe sampling permutation (mapper.cpp:1326-1333)."""
    idx = np.zeros(max(n, 1), np.int64)
    _chk(lib().sage_shuffle_indices(C.c_int64(seed), C.c_int64(n), idx.ctypes.data_as(C.POINTER(C.c_int64))),
         "sage_shuffle_indices")
    return idx[:n].copy()


def valid_locations(ws: "Workspace", mask, cam):
    """mask: [H,W] float cuda tensor; cam: SageCamera -> (loc1d int64 [n], homo [n,3]) cuda tensors."""
    import torch
    H, W = mask.shape
    loc = torch.zeros(H * W, dtype=torch.int64, device="cuda")
    homo = torch.zeros(H * W, 3, dtype=torch.float32, device="cuda")
    n = C.c_int()
    _chk(lib().sage_valid_locations(ws.h, C.c_void_p(mask.data_ptr()), C.byref(cam), C.c_void_p(loc.data_ptr()),
                                    C.c_void_p(homo.data_ptr()), C.byref(n)), "sage_valid_locations")
    return loc[:n.value].clone(), homo[:n.value].clone()


def sample_locations(ws: "Workspace", vloc, vhomo, seed: int, num_samples: int):
    import torch
    nv = int(vloc.shape[0])
    loc = torch.zeros(max(min(num_samples, nv), 1), dtype=torch.int64, device="cuda")
    homo = torch.zeros(max(min(num_samples, nv), 1), 3, dtype=torch.float32, device="cuda")
    n = C.c_int()
    _chk(lib().sage_sample_locations(ws.h, C.c_void_p(vloc.data_ptr()), C.c_void_p(vhomo.data_ptr()), nv,
                                     C.c_int64(seed), num_samples, C.c_void_p(loc.data_ptr()),
                                     C.c_void_p(homo.data_ptr()), C.byref(n)), "sage_sample_locations")
    return loc[:n.value].clone(), homo[:n.value].clone()


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bind_thread_to_device(device: int = 0) -> int:
    """``sage_bind_thread_to_device``: keep the calling thread on the GPU's NUMA node (returns the number of CPUs)."""
    return int(lib().sage_bind_thread_to_device(int(device)))


def solver_helper_cpus():
    """``sage_solver_helper_cpus``: CPUs the hybrid solve's helper threads are pinned to (-1: not placed yet)."""
    buf = (C.c_int * 3)()
    n = int(lib().sage_solver_helper_cpus(buf, 3))
    return [int(buf[i]) for i in range(n)]


def solver_placement_moves() -> int:
    """``sage_solver_placement_moves``: helpers the placement monitor has moved off crowded cores so far."""
    return int(lib().sage_solver_placement_moves())


def placement_monitor(enable: bool) -> None:
    """``sage_placement_monitor``: the background re-pinning of crowded helper threads is opt-in (r06)."""
    lib().sage_placement_monitor(1 if enable else 0)


def shutdown() -> None:
    """``sage_shutdown``: stop and join every host thread the library started (they restart on demand)."""
    lib().sage_shutdown()


def host_threads_running() -> int:
    """``sage_host_threads_running``: helper / pool / monitor threads of the library that are alive."""
    return int(lib().sage_host_threads_running())


def sort_locations(ws, loc1d, homo, H, W):
    """``sage_sort_locations``: raster-ordered copies of a keyframe's sampled locations -> (loc1d, homo, sorted?)."""
    import torch
    n = int(loc1d.shape[0])
    lo = torch.empty_like(loc1d)
    ho = torch.empty_like(homo)
    flag = C.c_int()
    _chk(lib().sage_sort_locations(ws.h, _dptr(loc1d), _dptr(homo), n, H, W, _dptr(lo), _dptr(ho), C.byref(flag)),
         "sage_sort_locations")
    return lo, ho, bool(flag.value)


def reprojection_jac_error(ws, R10, t10, R0, t0, R1, t1, bias0, basis0, code0, loc1d_i32, homo, matched, scale0, cam,
                           eps, loss_param, weight, CS):
    """All array arguments are cuda tensors (poses 9/3 floats).  Returns dict(AtA [D,D], Atb [D] tensors, error, num_inliers)."""
    import torch
    N = int(homo.shape[0]); D = 13 + CS
    AtA = torch.zeros(D, D, device="cuda"); Atb = torch.zeros(D, device="cuda")
    e = C.c_float(); n = C.c_float()
    _chk(lib().sage_reprojection_jac_error_calculate(
        ws.h, _dptr(AtA), _dptr(Atb), C.byref(e), C.byref(n), _dptr(R10), _dptr(t10), _dptr(R0), _dptr(t0), _dptr(R1),
        _dptr(t1), _dptr(bias0), _dptr(basis0), _dptr(code0), _dptr(loc1d_i32), _dptr(homo), _dptr(matched),
        C.c_float(scale0), C.byref(cam), C.c_float(eps), C.c_float(loss_param), C.c_float(weight), N, CS),
        "sage_reprojection_jac_error_calculate")
    return dict(AtA=AtA, Atb=Atb, error=e.value, num_inliers=n.value)


def reprojection_error(ws, R10, t10, bias0, basis0, code0, loc1d_i32, homo, matched, scale0, cam, eps, loss_param,
                       weight, CS):
    N = int(homo.shape[0])
    e = C.c_float(); n = C.c_float()
    _chk(lib().sage_reprojection_error_calculate(
        ws.h, C.byref(e), C.byref(n), _dptr(R10), _dptr(t10), _dptr(bias0), _dptr(basis0), _dptr(code0),
        _dptr(loc1d_i32), _dptr(homo), _dptr(matched), C.c_float(scale0), C.byref(cam), C.c_float(eps),
        C.c_float(loss_param), C.c_float(weight), N, CS), "sage_reprojection_error_calculate")
    return e.value, n.value


def tracker_reproj_jac_error(ws, R, t, dpts0, homo, matched, cam, eps, loss_param, weight):
    import torch
    N = int(homo.shape[0])
    AtA = torch.zeros(6, 6, device="cuda"); Atb = torch.zeros(6, device="cuda")
    e = C.c_float(); n = C.c_float()
    _chk(lib().sage_tracker_reproj_jac_error_calculate(
        ws.h, _dptr(AtA), _dptr(Atb), C.byref(e), C.byref(n), _dptr(R), _dptr(t), _dptr(dpts0), _dptr(homo),
        _dptr(matched), C.byref(cam), C.c_float(eps), C.c_float(loss_param), C.c_float(weight), N),
        "sage_tracker_reproj_jac_error_calculate")
    return dict(AtA=AtA, Atb=Atb, error=e.value, num_inliers=n.value)


def tracker_reproj_error(ws, R, t, dpts0, homo, matched, cam, eps, loss_param, weight):
    N = int(homo.shape[0])
    e = C.c_float(); n = C.c_float()
    _chk(lib().sage_tracker_reproj_error_calculate(
        ws.h, C.byref(e), C.byref(n), _dptr(R), _dptr(t), _dptr(dpts0), _dptr(homo), _dptr(matched), C.byref(cam),
        C.c_float(eps), C.c_float(loss_param), C.c_float(weight), N), "sage_tracker_reproj_error_calculate")
    return e.value, n.value


MG_LOSS = {"fair": 0, "L2": 1, "huber": 2, "unbiased": 3}


def match_geometry(ws, loss, jac, R10, t10, R0, t0, R1, t1, bias0, bias1, basis0, basis1, code0, code1, homo0, homo1,
                   loc0, loc1, scale0, scale1, loss_param, weight, CS):
    """Mapper match-geometry factor; cuda tensors in, dict(AtA, Atb, error) or the error out."""
    import torch
    N = int(homo0.shape[0]); D = 14 + 2 * CS
    e = C.c_float()
    if jac:
        AtA = torch.zeros(D, D, device="cuda"); Atb = torch.zeros(D, device="cuda")
        _chk(lib().sage_match_geometry_jac_error_calculate(
            ws.h, _dptr(AtA), _dptr(Atb), C.byref(e), _dptr(R10), _dptr(t10), _dptr(R0), _dptr(t0), _dptr(R1), _dptr(t1),
            _dptr(bias0), _dptr(bias1), _dptr(basis0), _dptr(basis1), _dptr(code0), _dptr(code1), _dptr(homo0),
            _dptr(homo1), _dptr(loc0), _dptr(loc1), C.c_float(scale0), C.c_float(scale1), C.c_float(loss_param),
            C.c_float(weight), MG_LOSS[loss], N, CS), "sage_match_geometry_jac_error_calculate")
        return dict(AtA=AtA, Atb=Atb, error=e.value)
    _chk(lib().sage_match_geometry_error_calculate(
        ws.h, C.byref(e), _dptr(R10), _dptr(t10), _dptr(bias0), _dptr(bias1), _dptr(basis0), _dptr(basis1), _dptr(code0),
        _dptr(code1), _dptr(homo0), _dptr(homo1), _dptr(loc0), _dptr(loc1), C.c_float(scale0), C.c_float(scale1),
        C.c_float(loss_param), C.c_float(weight), MG_LOSS[loss], N, CS), "sage_match_geometry_error_calculate")
    return e.value


def loop_mg(ws, jac, R10, t10, R0, t0, R1, t1, udpts0, udpts1, homo0, homo1, scale0, scale1, loss_param, weight):
    import torch
    N = int(homo0.shape[0])
    e = C.c_float()
    if jac:
        AtA = torch.zeros(14, 14, device="cuda"); Atb = torch.zeros(14, device="cuda")
        _chk(lib().sage_loop_mg_jac_error_calculate(
            ws.h, _dptr(AtA), _dptr(Atb), C.byref(e), _dptr(R10), _dptr(t10), _dptr(R0), _dptr(t0), _dptr(R1), _dptr(t1),
            _dptr(udpts0), _dptr(udpts1), _dptr(homo0), _dptr(homo1), C.c_float(scale0), C.c_float(scale1),
            C.c_float(loss_param), C.c_float(weight), N), "sage_loop_mg_jac_error_calculate")
        return dict(AtA=AtA, Atb=Atb, error=e.value)
    _chk(lib().sage_loop_mg_error_calculate(
        ws.h, C.byref(e), _dptr(R10), _dptr(t10), _dptr(udpts0), _dptr(udpts1), _dptr(homo0), _dptr(homo1),
        C.c_float(scale0), C.c_float(scale1), C.c_float(loss_param), C.c_float(weight), N), "sage_loop_mg_error_calculate")
    return e.value


def tracker_match_geom(ws, jac, with_scale, R, t, dpts0, dpts1, homo0, homo1, scale0, loss_param, weight):
    import torch
    N = int(homo0.shape[0]); D = 7 if with_scale else 6
    e = C.c_float()
    if jac:
        AtA = torch.zeros(D, D, device="cuda"); Atb = torch.zeros(D, device="cuda")
        _chk(lib().sage_tracker_match_geom_jac_error_calculate(
            ws.h, _dptr(AtA), _dptr(Atb), C.byref(e), _dptr(R), _dptr(t), _dptr(dpts0), _dptr(dpts1), _dptr(homo0),
            _dptr(homo1), C.c_float(scale0), C.c_float(loss_param), C.c_float(weight), int(with_scale), N),
            "sage_tracker_match_geom_jac_error_calculate")
        return dict(AtA=AtA, Atb=Atb, error=e.value)
    _chk(lib().sage_tracker_match_geom_error_calculate(
        ws.h, C.byref(e), _dptr(R), _dptr(t), _dptr(dpts0), _dptr(dpts1), _dptr(homo0), _dptr(homo1),
        C.c_float(loss_param), C.c_float(weight), N), "sage_tracker_match_geom_error_calculate")
    return e.value


def cycle_match(ws, desc0, desc1, kp_loc0, H, W, cyc_thresh):
    """desc0/desc1: [C,H,W] cuda float tensors; kp_loc0: int64 cuda tensor [K] -> (raw_matched1, cyc_matched0, flags, n)."""
    import torch
    K = int(kp_loc0.shape[0]); Cc = int(desc0.shape[0])
    m1 = torch.zeros(max(K, 1), dtype=torch.int64, device="cuda"); c0 = torch.zeros_like(m1)
    fl = torch.zeros(max(K, 1), dtype=torch.int32, device="cuda")
    n = C.c_int()
    _chk(lib().sage_cycle_match(ws.h, _dptr(desc0), _dptr(desc1), _dptr(kp_loc0), K, Cc, H, W, C.c_float(cyc_thresh),
                                _dptr(m1), _dptr(c0), _dptr(fl), C.byref(n)), "sage_cycle_match")
    return m1[:K], c0[:K], fl[:K], n.value


# --------------------------------------------------------------------------- robust registration of keypoint matches
SAGE_REG_MAX_POINTS = 1024
SAGE_REG_CHAIN, SAGE_REG_COMPLETE = 0, 1
SAGE_REG_SELECT_PMC_EXACT, SAGE_REG_SELECT_PMC_HEU, SAGE_REG_SELECT_KCORE_HEU, SAGE_REG_SELECT_NONE = range(4)
SAGE_REG_GNC_TLS, SAGE_REG_FGR = 0, 1


class SageRegistrationParams(C.Structure):
    _fields_ = [("noise_bound", C.c_double), ("cbar2", C.c_double), ("rotation_max_iterations", C.c_int),
                ("rotation_cost_threshold", C.c_double), ("rotation_gnc_factor", C.c_double), ("rotation_tim_graph", C.c_int),
                ("inlier_selection_mode", C.c_int), ("rotation_algorithm", C.c_int)]


class SageRegistrationResult(C.Structure):
    _fields_ = [("valid", C.c_int), ("scale", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("n_inliers", C.c_int),
                ("n_pairs", C.c_int), ("n_degenerate_pairs", C.c_int), ("n_scale_inlier_pairs", C.c_int),
                ("rotation_iterations", C.c_int), ("n_rotation_inliers", C.c_int), ("scale_cost", C.c_double)]


def registration_params(params=None, **kw) -> SageRegistrationParams:
    """a dict (``synth.registration_params``) and / or keywords -> ``SageRegistrationParams``; the reference's shipped values
    (configs/slam_run.flags:76-85) where nothing is given, noise_bound 0.01"""
    d = dict(noise_bound=0.01, cbar2=1.0, rotation_max_iterations=20, rotation_cost_threshold=1e-4, rotation_gnc_factor=1.4,
             rotation_tim_graph=SAGE_REG_CHAIN, inlier_selection_mode=SAGE_REG_SELECT_NONE, rotation_algorithm=SAGE_REG_GNC_TLS)
    d.update(params or {})
    d.update(kw)
    return SageRegistrationParams(**d)


def _reg_result(res: SageRegistrationResult) -> dict:
    out = {name: getattr(res, name) for name, _ in SageRegistrationResult._fields_ if name not in ("R", "t")}
    out["R"] = np.array(list(res.R), np.float64).reshape(3, 3)
    out["t"] = np.array(list(res.t), np.float64)
    return out


def robust_registration_raw(ws_handle, src_ptr, dst_ptr, nb_ptr, N, params_ptr, res_ptr, inliers_host_ptr, inliers_dev_ptr) -> int:
    """``sage_robust_registration`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_robust_registration
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(ws_handle, src_ptr, dst_ptr, nb_ptr, int(N), params_ptr, res_ptr, inliers_host_ptr, inliers_dev_ptr))


def robust_registration(ws: "Workspace", src, dst, noise_bounds, params=None, device_inliers: bool = False) -> dict:
    """``teaser::RobustRegistrationSolver::solve(src, dst, noise_bounds)`` in the reference's shipped configuration through
    ``sage_robust_registration``.  src, dst [N, 3], noise_bounds [N]: contiguous float32 cuda tensors; params: a dict, a
    ``SageRegistrationParams`` or None.  -> the fields of ``SageRegistrationResult`` (R [3, 3], t [3] float64 arrays) and
    ``inliers`` (int32 array, ascending); with ``device_inliers`` also ``inliers_dev`` (int32 cuda tensor [n_inliers])."""
    import torch
    N = int(src.shape[0])
    assert src.dtype == torch.float32 and dst.dtype == torch.float32 and noise_bounds.dtype == torch.float32
    assert tuple(dst.shape) == (N, 3) and noise_bounds.numel() == N
    p = params if isinstance(params, SageRegistrationParams) else registration_params(params)
    res = SageRegistrationResult()
    inl = np.zeros(max(N, 1), np.int32)
    inl_dev = torch.zeros(max(N, 1), dtype=torch.int32, device=src.device) if device_inliers else None
    _chk(robust_registration_raw(ws.h, dptr(src), dptr(dst), dptr(noise_bounds), N, C.addressof(p), C.addressof(res),
                                 inl.ctypes.data, dptr(inl_dev)), "sage_robust_registration")
    out = _reg_result(res)
    out["inliers"] = inl[:res.n_inliers].copy()
    if device_inliers:
        out["inliers_dev"] = inl_dev[:res.n_inliers]
    return out


def tls_estimate_raw(X_ptr, ranges_ptr, n, estimate_ptr, inliers_ptr) -> int:
    f = lib().sage_tls_estimate
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return int(f(X_ptr, ranges_ptr, int(n), estimate_ptr, inliers_ptr))


def tls_estimate(X, ranges):
    """``ScalarTLSEstimator::estimate`` through ``sage_tls_estimate`` (host, float64) -> (estimate, inliers [n] bool)"""
    X = np.ascontiguousarray(X, np.float64); ranges = np.ascontiguousarray(ranges, np.float64)
    assert X.ndim == 1 and X.shape == ranges.shape
    est = C.c_double()
    inl = np.zeros(max(X.size, 1), np.uint8)
    _chk(tls_estimate_raw(X.ctypes.data, ranges.ctypes.data, X.size, C.addressof(est), inl.ctypes.data), "sage_tls_estimate")
    return est.value, inl[:X.size].astype(bool)


def registration_finish_raw(src_ptr, dst_ptr, nb_ptr, N, scale, params_ptr, res_ptr, inliers_ptr, rotation_mask_ptr) -> int:
    f = lib().sage_registration_finish
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return int(f(src_ptr, dst_ptr, nb_ptr, int(N), float(scale), params_ptr, res_ptr, inliers_ptr, rotation_mask_ptr))


def registration_finish(src, dst, noise_bounds, scale: float, params=None) -> dict:
    """The solve's host finish for a given scale (chain TIMs, GNC-TLS rotation, translation votes) through
    ``sage_registration_finish``.  src, dst [N, 3], noise_bounds [N]: host arrays (taken as float32).  -> the result's fields,
    ``inliers`` (int32, ascending) and ``rotation_mask`` [N] bool"""
    src = _f32(src); dst = _f32(dst); nb = _f32(noise_bounds)
    N = int(src.shape[0])
    p = params if isinstance(params, SageRegistrationParams) else registration_params(params)
    res = SageRegistrationResult()
    inl = np.zeros(max(N, 1), np.int32); rot = np.zeros(max(N, 1), np.uint8)
    _chk(registration_finish_raw(src.ctypes.data, dst.ctypes.data, nb.ctypes.data, N, scale, C.addressof(p), C.addressof(res),
                                 inl.ctypes.data, rot.ctypes.data), "sage_registration_finish")
    out = _reg_result(res)
    out["inliers"] = inl[:res.n_inliers].copy()
    out["rotation_mask"] = rot[:N].astype(bool)
    return out


def match_points_raw(ws_handle, flags, loc1, dpts0, homo0, divisor0, dpt_map_1, cam_ptr, K, W, mult, noise_from, pts0, pts1, nb,
                     homo1, dpts1, kept, M_ptr, mean_ptr) -> int:
    """``sage_match_points`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_match_points
    f.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 8
    return int(f(ws_handle, flags, loc1, dpts0, homo0, float(divisor0), dpt_map_1, cam_ptr, int(K), int(W), float(mult),
                 int(noise_from), pts0, pts1, nb, homo1, dpts1, kept, M_ptr, mean_ptr))


def match_points(ws: "Workspace", flags, raw_matched_loc1, dpts0, homo0, depth_divisor0, dpt_map_1, cam, W, noise_multiplier,
                 noise_from: int = 1) -> dict:
    """The gather between ``sage_cycle_match`` and the solver through ``sage_match_points``.  flags [K] int32, raw_matched_loc1
    [K] int64, dpts0 [K], homo0 [K, 3], dpt_map_1 [H*W]: contiguous cuda tensors; cam: anything with fx, fy, cx, cy, w, h.
    -> dict(M, mean_depth, pts0, pts1 [M, 3], noise_bounds, dpts1 [M], homo1 [M, 3], kept [M] int32): cuda tensors cut to M."""
    import torch
    K = int(flags.numel())
    assert flags.dtype == torch.int32 and raw_matched_loc1.dtype == torch.int64
    c = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    dev = flags.device
    f3 = lambda: torch.zeros(max(K, 1), 3, dtype=torch.float32, device=dev)
    f1 = lambda: torch.zeros(max(K, 1), dtype=torch.float32, device=dev)
    pts0, pts1, homo1, nb, dpts1 = f3(), f3(), f3(), f1(), f1()
    kept = torch.zeros(max(K, 1), dtype=torch.int32, device=dev)
    M = C.c_int(); mean = C.c_float()
    _chk(match_points_raw(ws.h, dptr(flags), dptr(raw_matched_loc1), dptr(dpts0), dptr(homo0), depth_divisor0, dptr(dpt_map_1),
                          C.addressof(c), K, W, noise_multiplier, noise_from, dptr(pts0), dptr(pts1), dptr(nb), dptr(homo1),
                          dptr(dpts1), dptr(kept), C.addressof(M), C.addressof(mean)), "sage_match_points")
    m = M.value
    return dict(M=m, mean_depth=np.float32(mean.value), pts0=pts0[:m], pts1=pts1[:m], noise_bounds=nb[:m], homo1=homo1[:m],
                dpts1=dpts1[:m], kept=kept[:m])


# --------------------------------------------------------------------------- B registrations in one call
SAGE_REG_MAX_BATCH = 32


class SageRegistrationProblem(C.Structure):
    _fields_ = [("src_dev", C.c_void_p), ("dst_dev", C.c_void_p), ("noise_bounds_dev", C.c_void_p), ("N", C.c_int32),
                ("noise_bound", C.c_double), ("inliers_dev", C.c_void_p)]


class SageMatchPointsItem(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cyc_inlier_flags", "raw_matched_loc1d_1", "dpts0", "homo0", "dpt_map_1", "pts0", "pts1",
                                          "noise_bounds", "homo1", "dpts1", "kept")]


def robust_registration_batch_raw(ws_handle, probs_ptr, B, params_ptr, res_ptr, inliers_host_ptr, inliers_stride) -> int:
    """``sage_robust_registration_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_robust_registration_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return int(f(ws_handle, probs_ptr, int(B), params_ptr, res_ptr, inliers_host_ptr, int(inliers_stride)))


def robust_registration_batch_plan_raw(N_ptr, B, device_bytes_ptr, pinned_bytes_ptr, launches_ptr, order_ptr) -> int:
    f = lib().sage_robust_registration_batch_plan
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    return int(f(N_ptr, int(B), device_bytes_ptr, pinned_bytes_ptr, launches_ptr, order_ptr))


def robust_registration_batch_plan(N) -> dict:
    """What a batch of problems with these point counts will do, through ``sage_robust_registration_batch_plan`` (host only).
    -> dict(device_bytes, pinned_bytes, launches, order): ``order`` lists the rows of the voting problems (N >= 2) in the
    order of their segments (descending P, stable)."""
    n = np.ascontiguousarray(N, np.int32).reshape(-1)
    dev, pin = C.c_int64(), C.c_int64()
    launches = C.c_int32()
    order = np.full(max(n.size, 1), -1, np.int32)
    _chk(robust_registration_batch_plan_raw(n.ctypes.data if n.size else None, n.size, C.addressof(dev), C.addressof(pin),
                                            C.addressof(launches), order.ctypes.data), "sage_robust_registration_batch_plan")
    order = order[:n.size]
    return dict(device_bytes=dev.value, pinned_bytes=pin.value, launches=launches.value, order=[int(b) for b in order if b >= 0])


def robust_registration_batch_launches(ws: "Workspace") -> int:
    """the kernel launches of the workspace's last ``robust_registration_batch``"""
    f = lib().sage_robust_registration_batch_launches
    f.argtypes = [C.c_void_p]
    return int(f(ws.h))


def robust_registration_batch(ws: "Workspace", problems, params=None, device_inliers: bool = False) -> list:
    """B solves through ``sage_robust_registration_batch``.  problems: a list of dicts with ``src``, ``dst`` [N, 3],
    ``noise_bounds`` [N] (contiguous float32 cuda tensors; N may be 0 or 1) and ``noise_bound`` (the scalar bound of that
    problem); params: a dict, a ``SageRegistrationParams`` or None (its noise_bound is not read).  -> a list of B dicts as
    ``robust_registration`` returns them; row b equals that call on problem b alone."""
    import torch
    B = len(problems)
    p = params if isinstance(params, SageRegistrationParams) else registration_params(params)
    arr = (SageRegistrationProblem * max(B, 1))()
    res = (SageRegistrationResult * max(B, 1))()
    stride = max([int(q["src"].shape[0]) for q in problems] + [1])
    inl = np.zeros((max(B, 1), stride), np.int32)
    inl_dev = []
    for b, q in enumerate(problems):
        N = int(q["src"].shape[0])
        assert q["src"].dtype == torch.float32 and q["dst"].dtype == torch.float32 and q["noise_bounds"].dtype == torch.float32
        assert tuple(q["dst"].shape) == (N, 3) and q["noise_bounds"].numel() == N
        inl_dev.append(torch.zeros(max(N, 1), dtype=torch.int32, device="cuda") if device_inliers else None)
        arr[b] = SageRegistrationProblem(dptr(q["src"]).value, dptr(q["dst"]).value, dptr(q["noise_bounds"]).value, N,
                                         float(q["noise_bound"]), dptr(inl_dev[b]).value)
    _chk(robust_registration_batch_raw(ws.h, C.addressof(arr), B, C.addressof(p), C.addressof(res), inl.ctypes.data, stride),
         "sage_robust_registration_batch")
    out = []
    for b in range(B):
        o = _reg_result(res[b])
        o["inliers"] = inl[b, :res[b].n_inliers].copy()
        if device_inliers:
            o["inliers_dev"] = inl_dev[b][:res[b].n_inliers]
        out.append(o)
    return out


# --------------------------------------------------------------------------- the finish of a batch on the device
SAGE_REG_FINISH_HOST, SAGE_REG_FINISH_DEVICE = 0, 1
SAGE_REG_FINISH_MAX_ITERATIONS = 1000


def workspace_set_registration_finish_raw(ws_handle, mode) -> int:
    f = lib().sage_workspace_set_registration_finish
    f.argtypes = [C.c_void_p, C.c_int]
    return int(f(ws_handle, int(mode)))


def workspace_registration_finish_raw(ws_handle) -> int:
    f = lib().sage_workspace_registration_finish
    f.argtypes = [C.c_void_p]
    return int(f(ws_handle))


def registration_finish_batch_raw(ws_handle, probs_ptr, B, scales_ptr, params_ptr, res_ptr, inliers_host_ptr, inliers_stride,
                                  rotation_masks_ptr) -> int:
    """``sage_registration_finish_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_registration_finish_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return int(f(ws_handle, probs_ptr, int(B), scales_ptr, params_ptr, res_ptr, inliers_host_ptr, int(inliers_stride), rotation_masks_ptr))


def registration_finish_batch(ws: "Workspace", problems, scales, params=None, device_inliers: bool = False) -> list:
    """The finish of B solves for given scales on the device through ``sage_registration_finish_batch``.  problems: as
    ``robust_registration_batch`` takes them; scales: B floats.  -> a list of B dicts as ``registration_finish`` returns them
    (``inliers``, ``rotation_mask`` [N] bool; with ``device_inliers`` also ``inliers_dev``)."""
    import torch
    B = len(problems)
    p = params if isinstance(params, SageRegistrationParams) else registration_params(params)
    arr = (SageRegistrationProblem * max(B, 1))()
    res = (SageRegistrationResult * max(B, 1))()
    sc = np.ascontiguousarray(scales, np.float64).reshape(-1)
    assert sc.size == B
    stride = max([int(q["src"].shape[0]) for q in problems] + [1])
    inl = np.zeros((max(B, 1), stride), np.int32); rot = np.zeros((max(B, 1), stride), np.uint8)
    inl_dev = []
    for b, q in enumerate(problems):
        N = int(q["src"].shape[0])
        assert q["src"].dtype == torch.float32 and q["dst"].dtype == torch.float32 and q["noise_bounds"].dtype == torch.float32
        assert tuple(q["dst"].shape) == (N, 3) and q["noise_bounds"].numel() == N
        inl_dev.append(torch.zeros(max(N, 1), dtype=torch.int32, device="cuda") if device_inliers else None)
        arr[b] = SageRegistrationProblem(dptr(q["src"]).value, dptr(q["dst"]).value, dptr(q["noise_bounds"]).value, N,
                                         float(q["noise_bound"]), dptr(inl_dev[b]).value)
    _chk(registration_finish_batch_raw(ws.h, C.addressof(arr), B, sc.ctypes.data if B else None, C.addressof(p), C.addressof(res),
                                       inl.ctypes.data, stride, rot.ctypes.data), "sage_registration_finish_batch")
    out = []
    for b, q in enumerate(problems):
        o = _reg_result(res[b])
        o["inliers"] = inl[b, :res[b].n_inliers].copy()
        o["rotation_mask"] = rot[b, :int(q["src"].shape[0])].astype(bool)
        if device_inliers:
            o["inliers_dev"] = inl_dev[b][:res[b].n_inliers]
        out.append(o)
    return out


def registration_finish_plan_raw(N_ptr, B, launches_ptr, pinned_bytes_ptr, lds_bytes_ptr, workgroups_ptr) -> int:
    f = lib().sage_registration_finish_plan
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    return int(f(N_ptr, int(B), launches_ptr, pinned_bytes_ptr, lds_bytes_ptr, workgroups_ptr))


def registration_finish_plan(N) -> dict:
    """What ``robust_registration_batch`` will do for these point counts in ``SAGE_REG_FINISH_DEVICE`` mode, through
    ``sage_registration_finish_plan`` (host only) -> dict(launches, pinned_bytes, lds_bytes, workgroups)"""
    n = np.ascontiguousarray(N, np.int32).reshape(-1)
    launches, lds, wgs = C.c_int32(), C.c_int32(), C.c_int32()
    pin = C.c_int64()
    _chk(registration_finish_plan_raw(n.ctypes.data if n.size else None, n.size, C.addressof(launches), C.addressof(pin),
                                      C.addressof(lds), C.addressof(wgs)), "sage_registration_finish_plan")
    return dict(launches=launches.value, pinned_bytes=pin.value, lds_bytes=lds.value, workgroups=wgs.value)


def match_points_batch_raw(ws_handle, items_ptr, B, divisor0, cam_ptr, K, W, mult, noise_from, M_ptr, mean_ptr) -> int:
    """``sage_match_points_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_match_points_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    return int(f(ws_handle, items_ptr, int(B), float(divisor0), cam_ptr, int(K), int(W), float(mult), int(noise_from), M_ptr, mean_ptr))


def match_points_batch(ws: "Workspace", problems, depth_divisor0, cam, W, noise_multiplier, noise_from: int = 1) -> list:
    """B gathers through ``sage_match_points_batch``.  problems: a list of dicts with ``flags`` [K] int32, ``raw_matched_loc1``
    [K] int64, ``dpts0`` [K], ``homo0`` [K, 3], ``dpt_map_1`` [H*W] (contiguous cuda tensors, one K for all).  -> a list of B
    dicts as ``match_points`` returns them, and under ``full`` the uncut output tensors (zero where nothing was written)."""
    import torch
    B = len(problems)
    K = int(problems[0]["flags"].numel()) if B else 1
    c = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    items = (SageMatchPointsItem * max(B, 1))()
    outs = []
    for b, q in enumerate(problems):
        assert q["flags"].dtype == torch.int32 and q["raw_matched_loc1"].dtype == torch.int64 and int(q["flags"].numel()) == K
        dev = q["flags"].device
        o = dict(pts0=torch.zeros(K, 3, dtype=torch.float32, device=dev), pts1=torch.zeros(K, 3, dtype=torch.float32, device=dev),
                 noise_bounds=torch.zeros(K, dtype=torch.float32, device=dev), homo1=torch.zeros(K, 3, dtype=torch.float32, device=dev),
                 dpts1=torch.zeros(K, dtype=torch.float32, device=dev), kept=torch.zeros(K, dtype=torch.int32, device=dev))
        outs.append(o)
        items[b] = SageMatchPointsItem(*[dptr(t).value for t in (q["flags"], q["raw_matched_loc1"], q["dpts0"], q["homo0"], q["dpt_map_1"],
                                                                 o["pts0"], o["pts1"], o["noise_bounds"], o["homo1"], o["dpts1"], o["kept"])])
    M = np.zeros(max(B, 1), np.int32); mean = np.zeros(max(B, 1), np.float32)
    _chk(match_points_batch_raw(ws.h, C.addressof(items), B, depth_divisor0, C.addressof(c), K, W, noise_multiplier, noise_from,
                                M.ctypes.data, mean.ctypes.data), "sage_match_points_batch")
    res = []
    for b in range(B):
        m = int(M[b])
        r = {k: v[:m] for k, v in outs[b].items()}
        r.update(M=m, mean_depth=np.float32(mean[b]), full=outs[b])
        res.append(r)
    return res


# --------------------------------------------------------------------------- the loop detector's candidates in one call
SAGE_MATCH_MAX_BATCH = 32


class SageLoopCandidate(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("desc_dev", "dpt_map_dev", "kp_loc1d_dev", "kp_dpts0_dev", "kp_homo0_dev")]


class SageLoopPrecheckResult(C.Structure):
    _fields_ = [("n_cycle", C.c_int32), ("n_matched", C.c_int32), ("registered", C.c_int32),
                ("relative_desc_match_inlier_ratio", C.c_float), ("desc_match_inlier_ratio", C.c_float),
                ("mean_noise_depth", C.c_float), ("reg", SageRegistrationResult)]


def cycle_match_batch_raw(ws_handle, desc_q, cand_ptrs, kp_ptrs, B, K, Cc, H, W, cyc_thresh, pixel_slices, raw, cyc, flags,
                          counts_ptr) -> int:
    """``sage_cycle_match_batch`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_cycle_match_batch
    f.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.c_float, C.c_int] + [C.c_void_p] * 4
    return int(f(ws_handle, desc_q, cand_ptrs, kp_ptrs, int(B), int(K), int(Cc), int(H), int(W), float(cyc_thresh),
                 int(pixel_slices), raw, cyc, flags, counts_ptr))


def _ptr_array(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[int(t.data_ptr()) for t in tensors])


def cycle_match_batch(ws, desc_q, desc_cands, kp_locs, H, W, cyc_thresh, pixel_slices: int = 0):
    """One query map against B candidate maps through ``sage_cycle_match_batch``.  desc_q [C,H,W] and every desc_cands[b]:
    contiguous cuda float tensors; kp_locs[b]: int64 cuda tensor [K] (candidate b's keypoints, pixels of the query map).
    -> (raw_matched [B,K], cyc_matched [B,K], flags [B,K] int32, counts [B] numpy int32, the number of pixel slices used);
    row b is what ``cycle_match(ws, desc_q, desc_cands[b], kp_locs[b], ...)`` returns."""
    import torch
    B = len(desc_cands)
    assert len(kp_locs) == B
    K = int(kp_locs[0].shape[0]) if B else 0
    Cc = int(desc_q.shape[0])
    for d, k in zip(desc_cands, kp_locs):
        assert d.is_contiguous() and k.is_contiguous() and k.dtype == torch.int64 and int(k.shape[0]) == K and tuple(d.shape) == tuple(desc_q.shape)
    raw = torch.zeros(max(B, 1), max(K, 1), dtype=torch.int64, device="cuda"); cyc = torch.zeros_like(raw)
    fl = torch.zeros(max(B, 1), max(K, 1), dtype=torch.int32, device="cuda")
    counts = np.zeros(max(B, 1), np.int32)
    _chk(cycle_match_batch_raw(ws.h, dptr(desc_q), _ptr_array(desc_cands), _ptr_array(kp_locs), B, K, Cc, H, W, cyc_thresh,
                               pixel_slices, dptr(raw), dptr(cyc), dptr(fl), counts.ctypes.data), "sage_cycle_match_batch")
    f = lib().sage_cycle_match_batch_slices
    f.argtypes = [C.c_void_p]
    return raw[:B, :K], cyc[:B, :K], fl[:B, :K], counts[:B], int(f(ws.h))


def loop_precheck_raw(ws_handle, desc_q, divisor, cands_ptr, B, K, Cc, H, W, cam_ptr, cyc_thresh, mult, min_ratio, params_ptr,
                      results_ptr, raw, flags, inlier_kp) -> int:
    """``sage_loop_precheck`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_loop_precheck
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] + [C.c_float] * 3 + [C.c_void_p] * 5
    return int(f(ws_handle, desc_q, float(divisor), cands_ptr, int(B), int(K), int(Cc), int(H), int(W), cam_ptr, float(cyc_thresh),
                 float(mult), float(min_ratio), params_ptr, results_ptr, raw, flags, inlier_kp))


def loop_precheck(ws, desc_q, query_depth_divisor, cands, H, W, cam, cyc_thresh, noise_multiplier, min_desc_inlier_ratio,
                  params=None):
    """The loop detector's pre-check of B candidates through ``sage_loop_precheck``.  desc_q [C,H,W]; cands: a list of dicts with
    the contiguous cuda tensors ``desc`` [C,H,W], ``dpt_map`` [H*W], ``kp_loc`` [K] int64, ``kp_dpts0`` [K], ``kp_homo0`` [K,3];
    cam: anything with fx, fy, cx, cy, w, h; params: a dict, a ``SageRegistrationParams`` or None (noise_bound is not read).
    -> a list of B dicts: n_cycle, n_matched, registered, the two ratios, mean_noise_depth, ``reg`` (the fields of
    ``SageRegistrationResult``), ``raw_matched`` [K] int64, ``flags`` [K] int32, ``inlier_kp`` [reg.n_inliers] int32 (cuda)."""
    import torch
    B = len(cands)
    K = int(cands[0]["kp_loc"].shape[0]) if B else 0
    Cc = int(desc_q.shape[0])
    arr = (SageLoopCandidate * max(B, 1))()
    for b, c in enumerate(cands):
        assert c["kp_loc"].dtype == torch.int64 and int(c["kp_loc"].shape[0]) == K and tuple(c["kp_homo0"].shape) == (K, 3)
        arr[b] = SageLoopCandidate(*[dptr(c[n]).value for n in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")])
    c = SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)])
    p = params if isinstance(params, SageRegistrationParams) else registration_params(params)
    res = (SageLoopPrecheckResult * max(B, 1))()
    raw = torch.zeros(max(B, 1), max(K, 1), dtype=torch.int64, device="cuda")
    fl = torch.zeros(max(B, 1), max(K, 1), dtype=torch.int32, device="cuda")
    ikp = torch.zeros(max(B, 1), max(K, 1), dtype=torch.int32, device="cuda")
    _chk(loop_precheck_raw(ws.h, dptr(desc_q), query_depth_divisor, C.addressof(arr), B, K, Cc, H, W, C.addressof(c), cyc_thresh,
                           noise_multiplier, min_desc_inlier_ratio, C.addressof(p), C.addressof(res), dptr(raw), dptr(fl), dptr(ikp)),
         "sage_loop_precheck")
    out = []
    for b in range(B):
        r = res[b]
        out.append(dict(n_cycle=r.n_cycle, n_matched=r.n_matched, registered=r.registered,
                        relative_desc_match_inlier_ratio=np.float32(r.relative_desc_match_inlier_ratio),
                        desc_match_inlier_ratio=np.float32(r.desc_match_inlier_ratio),
                        mean_noise_depth=np.float32(r.mean_noise_depth), reg=_reg_result(r.reg), raw_matched=raw[b, :K],
                        flags=fl[b, :K], inlier_kp=ikp[b, :r.reg.n_inliers]))
    return out


class SageLoopVerifyQuery(C.Structure):
    _fields_ = [("N", C.c_int32), ("FS", C.c_int32), ("homo_dev", C.c_void_p), ("unscaled_dpts0_dev", C.c_void_p),
                ("feat0s_dev", C.c_void_p), ("weights_dev", C.c_void_p), ("pyr", SagePyramid), ("eps", C.c_float), ("M", C.c_int32),
                ("valid_homo_dev", C.c_void_p), ("valid_dpts0_dev", C.c_void_p), ("mask_dev", C.c_void_p)]


class SageLoopVerifyCandidate(C.Structure):
    _fields_ = [("feat1_dev", C.c_void_p), ("grad1_dev", C.c_void_p), ("mask1_dev", C.c_void_p), ("kp_loss_param", C.c_float)]


class SageLoopVerifyResult(C.Structure):
    _fields_ = [("tracked", C.c_int32), ("status", C.c_int32), ("pose12", C.c_float * 12), ("scale", C.c_float),
                ("error", C.c_float), ("iters", C.c_int32), ("area_ratio", C.c_float), ("inlier_ratio", C.c_float),
                ("average_motion", C.c_float), ("area_inlier_ratio", C.c_float)]


def loop_verify_raw(ws_handle, cfg_ptr, query_ptr, divisor, cands_ptr, vcands_ptr, pre_ptr, B, K, raw, inlier_kp, mg_weight, gathered,
                    results_ptr) -> int:
    """``sage_loop_verify`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_loop_verify
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                  C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    return int(f(ws_handle, cfg_ptr, query_ptr, float(divisor), cands_ptr, vcands_ptr, pre_ptr, int(B), int(K), raw, inlier_kp,
                 float(mg_weight), gathered, results_ptr))


def loop_verify(ws, cfg: SageLmConfig, query: SageLoopVerifyQuery, query_depth_divisor, cands, vcands, pre, raw_matched, inlier_kp,
                match_geom_factor_weight):
    """The loop detector's body after the ratio test through ``sage_loop_verify``.  cands: the dicts of ``loop_precheck``;
    vcands: dicts with the cuda tensors ``feat1``, ``grad1``, ``mask1`` and the float ``kp_loss_param``; pre: a ctypes array of
    ``SageLoopPrecheckResult`` [B]; raw_matched [B,K] int64, inlier_kp [B,K] int32: cuda tensors as the pre-check wrote them.
    -> (a ctypes array of B ``SageLoopVerifyResult``, the gathered keypoint terms: a [B, 8 K] cuda tensor, row b = homo0 [K,3] |
    unscaled dpts0 [K] | homo1 [K,3] | dpts1 [K])."""
    import torch
    B = len(cands)
    K = int(raw_matched.shape[1]) if B else 0
    arr = (SageLoopCandidate * max(B, 1))()
    varr = (SageLoopVerifyCandidate * max(B, 1))()
    for b, (c, v) in enumerate(zip(cands, vcands)):
        arr[b] = SageLoopCandidate(*[dptr(c[n]).value for n in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")])
        varr[b] = SageLoopVerifyCandidate(dptr(v["feat1"]).value, dptr(v["grad1"]).value, dptr(v["mask1"]).value,
                                          float(v["kp_loss_param"]))
    res = (SageLoopVerifyResult * max(B, 1))()
    gathered = torch.zeros(max(B, 1), 8 * max(K, 1), dtype=torch.float32, device="cuda")
    _chk(loop_verify_raw(ws.h, C.addressof(cfg), C.addressof(query), query_depth_divisor, C.addressof(arr), C.addressof(varr),
                         C.addressof(pre), B, K, dptr(raw_matched), dptr(inlier_kp), match_geom_factor_weight, dptr(gathered),
                         C.addressof(res)), "sage_loop_verify")
    return res, gathered


class SageLoopAcceptConfig(C.Structure):
    _fields_ = [("min_area_ratio", C.c_float), ("min_inlier_ratio", C.c_float), ("base_metric", C.c_float),
                ("base_desc_ratio", C.c_float), ("redundant_range", C.c_int64), ("dpt_eps", C.c_float)]


class SageLoopScaleQuery(C.Structure):
    _fields_ = [("bias_dev", C.c_void_p), ("video_mask_dev", C.c_void_p), ("cam", SageCamera)]


class SageLoopScaleCandidate(C.Structure):
    _fields_ = [("id", C.c_int64), ("valid_loc1d_dev", C.c_void_p), ("valid_homo_dev", C.c_void_p), ("M", C.c_int32),
                ("dpt_scale", C.c_float), ("tracker_ref_scale", C.c_float)]


class SageLoopInfo(C.Structure):
    _fields_ = [("accepted", C.c_int32), ("kept", C.c_int32), ("id_ref", C.c_int64), ("R_cur_ref", C.c_float * 9),
                ("t_cur_ref", C.c_float * 3), ("query_scale", C.c_float), ("ref_scale", C.c_float),
                ("desc_inlier_ratio", C.c_float), ("metric", C.c_float), ("scale", SageDepthScaleStats)]


def loop_accept_raw(ws_handle, cfg_ptr, query_ptr, cands_ptr, scands_ptr, pre_ptr, ver_ptr, B, infos_ptr, kept_ptr, n_kept_ptr) -> int:
    """``sage_loop_accept`` with the arguments as given (handles / pointers may be None) -> status code"""
    f = lib().sage_loop_accept
    f.argtypes = [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 3
    return int(f(ws_handle, cfg_ptr, query_ptr, cands_ptr, scands_ptr, pre_ptr, ver_ptr, int(B), infos_ptr, kept_ptr, n_kept_ptr))


def loop_accept(ws, cfg: SageLoopAcceptConfig, query_bias, query_mask, cam, cands, scands, pre, ver):
    """The loop detector's accept test, pose hand-over, depth-scale correction, sort and redundancy filter through
    ``sage_loop_accept``.  query_bias, query_mask [h,w]: cuda tensors of the keyframe to scale, cam: its level-0 camera; cands:
    the dicts of ``loop_precheck`` (``dpt_map`` is read); scands: dicts with ``id``, the cuda tensors ``valid_loc1d`` [M] int64
    and ``valid_homo`` [M,3], and the floats ``dpt_scale``, ``tracker_ref_scale``; pre, ver: the ctypes arrays of
    ``SageLoopPrecheckResult`` / ``SageLoopVerifyResult`` [B].
    -> (a ctypes array of B ``SageLoopInfo`` in candidate order, the kept candidates' indices in the reference's order)."""
    B = len(cands)
    arr = (SageLoopCandidate * max(B, 1))()
    sarr = (SageLoopScaleCandidate * max(B, 1))()
    for b, (c, s) in enumerate(zip(cands, scands)):
        arr[b] = SageLoopCandidate(*[dptr(c.get(n)).value for n in ("desc", "dpt_map", "kp_loc", "kp_dpts0", "kp_homo0")])
        sarr[b] = SageLoopScaleCandidate(int(s["id"]), dptr(s["valid_loc1d"]).value, dptr(s["valid_homo"]).value,
                                         int(s["valid_homo"].shape[0]), float(s["dpt_scale"]), float(s["tracker_ref_scale"]))
    q = SageLoopScaleQuery(dptr(query_bias).value, dptr(query_mask).value,
                           SageCamera(*[float(v) for v in (cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h)]))
    infos = (SageLoopInfo * max(B, 1))()
    kept = (C.c_int32 * max(B, 1))()
    n_kept = C.c_int32()
    _chk(loop_accept_raw(ws.h, C.addressof(cfg), C.addressof(q), C.addressof(arr), C.addressof(sarr), C.addressof(pre),
                         C.addressof(ver), B, C.addressof(infos), C.addressof(kept), C.addressof(n_kept)), "sage_loop_accept")
    return infos, [int(kept[i]) for i in range(n_kept.value)]


# ----------------------------------------------------------------------------------------------------------------------
# keyframe ingest: the outputs of the (TorchScript) feature / depth networks -> the tensor bundle of a keyframe, on the
# device end to end (what Mapper::BuildKeyframe does with libtorch ops, core/mapping/mapper.cpp:1318-1426, 1242-1252)
# ----------------------------------------------------------------------------------------------------------------------
class IngestedKeyframe:
    """device tensors of one keyframe in the reference layouts (a10) + the host-side variables; duck-types a
    ``synth.Keyframe`` for :class:`Window` / :class:`DeviceKeyframe` (no host copy is made of the big tensors)."""

    def __init__(self, feat_pyr, grad_pyr, bias, basis, loc1d, homo, R, t, code, scale, avg_squared_dpt_bias):
        self.feat_pyr, self.grad_pyr, self.bias, self.basis = feat_pyr, grad_pyr, bias, basis
        self.loc1d, self.homo = loc1d, homo
        self.R, self.t, self.code, self.scale = R, t, code, scale
        self.avg_squared_dpt_bias = avg_squared_dpt_bias


def keyframe_from_net_outputs(ws: "Workspace", feat_map, dpt_bias, dpt_jac_code, mask, pyr: SagePyramid, seed: int,
                              num_samples: int, R=None, t=None):
    """feat_map [1,FS,H,W] or [FS,H,W] (feature net), dpt_bias [1,1,H,W] or [H,W], dpt_jac_code [H*W,CS] (depth net),
    mask [H,W] float 0/1 -- CUDA tensors that stay where they are.  Masked Gaussian pyramid + central-difference
    gradients (mapper.cpp:1384-1426), valid-pixel enumeration (mapping_utils.h:254-287), seeded std::shuffle subsample
    with seed = timestamp (mapper.cpp:1326-1340), zero initial code, unit scale (mapper.cpp:1242, :1318)."""
    import torch
    feat = feat_map.reshape(feat_map.shape[-3], feat_map.shape[-2], feat_map.shape[-1]).contiguous().float()
    FS, H, W = feat.shape
    bias = dpt_bias.reshape(-1).contiguous().float()
    basis = dpt_jac_code.reshape(H * W, -1).contiguous().float()
    CS = int(basis.shape[1])
    assert bias.numel() == H * W and mask.shape == (H, W)
    feat_pyr, grad_pyr = gaussian_pyramid_with_grad(ws, feat, mask, pyr, FS)
    vloc, vhomo = valid_locations(ws, mask, pyr.cam[0])
    loc, homo = sample_locations(ws, vloc, vhomo, seed, num_samples)
    # avg_squared_dpt_bias (mapper.cpp:1248-1250): the per-link Cauchy parameter of the geometric factor derives from it
    avg = float((torch.sum(torch.square(bias * mask.reshape(-1))) / torch.sum(mask)).item())
    R = np.eye(3, dtype=np.float32) if R is None else np.asarray(R, np.float32)
    t = np.zeros(3, np.float32) if t is None else np.asarray(t, np.float32)
    return IngestedKeyframe(feat_pyr, grad_pyr, bias, basis, loc, homo, R, t, np.zeros(CS, np.float32), 1.0, avg)
