/*
 * sage_ba.h -- C ABI of the MI355X-native dense bundle-adjustment engine.
 *
 * This is the drop-in boundary for the hot path of lppllppl920/SAGE-SLAM: the
 * per-pixel feature-metric (photometric) and geometric residual/Jacobian
 * evaluation and the Gauss-Newton/LM reduction into the pose x depth-code x
 * scale normal equations.  It replaces the free functions declared in
 *     system/sources/cuda/photometric_factor_kernels.h
 *     system/sources/cuda/geometric_factor_kernels.h
 * (namespace df, templated on CS/FS) and adds the batched window engine the
 * reference does not have (one launch over all factor-graph edges, block-sparse
 * normal equations, edge sharding across GPUs).
 *
 * Conventions
 *   - every `dev` pointer is a plain HIP device pointer (fp32 unless noted);
 *     layouts are the reference's own: feature pyramids
 *     [FS,P] channel-major with levels concatenated fine->coarse, gradient
 *     pyramids [2,FS,P] (x then y), bias [H*W], basis [H*W,CS] row-major,
 *     mask [H,W] float 0/1, homo [N,3], loc1d [N].
 *   - poses are world-from-keyframe; a pose buffer is 12 floats: R row-major
 *     (9) then t (3).  Tangent order [translation(3), rotation(3)], update is a
 *     LEFT multiplication T <- exp(delta)*T  (core/gtsam/gtsam_traits.h:45-70).
 *   - no torch types, no exceptions; every function returns 0 on success or a
 *     negative SAGE_E_* / positive hipError_t code (the reference calls exit()
 *     on a launch error: photometric_factor_kernels.cpp:18-31).
 *   - "no inliers" is NOT an error: error = 10*sum(w) (photometric) or
 *     10*weight (geometric), AtA = Atb = 0 (photometric...cpp:1156-1161,
 *     geometric...cpp:942-947).
 *   - all entry points are re-entrant; a SageWorkspace (stream + scratch) must
 *     not be used from two host threads at once (the reference is called from
 *     up to 4 host threads: deepfactors.cpp:1497-1505 -> one workspace each).
 *
 * The product path has no CPU fallback: without a HIP device every compute
 * entry point fails with the hipError from the runtime.
 */
#ifndef SAGE_BA_H_
#define SAGE_BA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAGE_MAX_LEVELS 8
#define SAGE_POSE_FLOATS 12 /* R (9, row-major) then t (3) */

#define SAGE_OK 0
#define SAGE_E_INVALID (-1)     /* bad argument (null pointer, unsupported CS/FS/L ...) */
#define SAGE_E_UNSUPPORTED (-2) /* combination not instantiated */
#define SAGE_E_NOT_PSD (-3)     /* host solve: matrix not positive definite even after damping */
#define SAGE_E_STATE (-4)       /* call order violated (e.g. solve before linearize) */
#define SAGE_E_NO_OVERLAP (-5)  /* tracker LM: "no overlap between frame to track and keyframe" (camera_tracker.cpp:1515-1519; the reference returns false) */

/* ---- cameras: replaces df::PinholeCamera<float> / df::CameraPyramid<float>
 *      (common/pinhole_camera.h:44-131, common/camera_pyramid.h:18-32) ---- */
typedef struct SageCamera
{
  float fx, fy, cx, cy, w, h;
} SageCamera;

typedef struct SagePyramid
{
  int32_t levels;
  int32_t P; /* total texels over all levels */
  int32_t level_offsets[SAGE_MAX_LEVELS];
  SageCamera cam[SAGE_MAX_LEVELS];
} SagePyramid;

/* CameraPyramid ctor: level i = level i-1 resized to (size_t)(w/2),(size_t)(h/2). Host only. */
/* (Level coordinates: a pyramid whose per-level focal ratios fx_l/fx_0, fy_l/fy_0 are exact powers of two -- every pyramid
 * this function / the reference's CameraPyramid builds while the level sizes stay even, i.e. the only sizes for which the
 * reference's own conv / camera / mask pyramids agree -- is sampled with the host-side quotient (bit-identical to the
 * reference's ((p + 0.5) * fx_l) / fx_0 - 0.5, photometric_factor_kernels.cpp:101-103, there).  r06: any other pyramid (an odd
 * level size, w = 250 -> 125 -> 62, or hand-made focal lengths) is accepted too: the kernels then evaluate the reference's
 * expression per pixel -- true multiplication, true division -- on the texture-path sampler; slower, same results.) */
int sage_camera_pyramid(const SageCamera *base, int levels, SagePyramid *out);

const char *sage_version(void);
const char *sage_error_string(int code);

/* ---- workspace: one per host thread / stream ---- */
typedef struct SageWorkspace SageWorkspace;
/* hip_stream: a hipStream_t (NULL = default stream). */
int sage_workspace_create(void *hip_stream, SageWorkspace **out);
void sage_workspace_destroy(SageWorkspace *ws);

/* =====================================================================
 * Per-edge operator API == the reference's free functions, raw pointers.
 * AtA/Atb are DEVICE outputs (row-major D x D and D), `error` is a HOST
 * output (the call synchronises the stream, like the reference's .item()).
 * ===================================================================== */

/* df::photometric_jac_error_calculate<CS,FS>  (photometric_factor_kernels.h:20-33,
 * .cpp:1061-1164).  D = 13+CS, column order [pose0(6) pose1(6) code0(CS) scale0].
 * weights: HOST float[L] (the reference passes a CPU tensor: photometric_factor.cpp:31-32). */
int sage_photometric_jac_error_calculate(
    SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host, float *num_inliers_host,
    const float *R10_dev, const float *t10_dev, const float *R0_dev, const float *t0_dev,
    const float *R1_dev, const float *t1_dev,
    const float *bias0_dev, const float *basis0_dev, const float *code0_dev, const float *mask1_dev,
    const int64_t *loc1d_dev, const float *homo_dev,
    const float *feat0_dev, const float *feat1_dev, const float *grad1_dev,
    float scale0, const SagePyramid *pyr, float eps, const float *weights_host,
    int N, int FS, int CS);

/* df::photometric_error_calculate<FS>  (photometric_factor_kernels.h:9-18, .cpp:990-1059) */
int sage_photometric_error_calculate(
    SageWorkspace *ws, float *error_host, float *num_inliers_host,
    const float *R10_dev, const float *t10_dev,
    const float *bias0_dev, const float *basis0_dev, const float *code0_dev, const float *mask1_dev,
    const int64_t *loc1d_dev, const float *homo_dev,
    const float *feat0_dev, const float *feat1_dev,
    float scale0, const SagePyramid *pyr, float eps, const float *weights_host,
    int N, int FS, int CS);

/* df::tracker_photo_jac_error_calculate<FS> (dof = 6, photometric_factor_kernels.h:35-46, .cpp:1166-1245)
 * df::tracker_photo_jac_error_calculate_with_scale<FS> (dof = 7, .h:48-59, .cpp:1247-1325).
 * feat0s = pre-sampled source features [L,N,FS]; weights: DEVICE float[L] (tracker passes a device tensor). */
int sage_tracker_photo_jac_error_calculate(
    SageWorkspace *ws, int dof, float *AtA_dev, float *Atb_dev, float *error_host, float *num_inliers_host,
    const float *R_dev, const float *t_dev, const float *mask1_dev,
    const float *dpts0_dev, const float *homo_dev, const float *feat0s_dev,
    const float *feat1_dev, const float *grad1_dev,
    const SagePyramid *pyr, float scale0, float eps, const float *weights_dev, int N, int FS);

/* df::tracker_photo_error_calculate<FS> (photometric_factor_kernels.h:61-70, .cpp:1327-1384) */
int sage_tracker_photo_error_calculate(
    SageWorkspace *ws, float *error_host, float *num_inliers_host,
    const float *R_dev, const float *t_dev, const float *mask1_dev,
    const float *dpts0_dev, const float *homo_dev, const float *feat0s_dev, const float *feat1_dev,
    const SagePyramid *pyr, float eps, const float *weights_dev, int N, int FS);

/* df::geometric_jac_error_calculate<CS> (geometric_factor_kernels.h:38-48, .cpp:882-950).
 * D = 14+2CS, column order [pose0 pose1 code0 code1 scale0 scale1].  dpt1 = s1*(bias1+basis1*code1) [H,W],
 * dpt_grad1 [2,H,W], basis1 [H,W,CS]; loc1d is int32 here (geometric_factor.cpp:344). */
int sage_geometric_jac_error_calculate(
    SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host, float *num_inliers_host,
    const float *R10_dev, const float *t10_dev, const float *R0_dev, const float *t0_dev,
    const float *R1_dev, const float *t1_dev,
    const float *bias0_dev, const float *basis0_dev, const float *code0_dev,
    const float *dpt1_dev, const float *dpt_grad1_dev, const float *basis1_dev, const float *mask1_dev,
    const int32_t *loc1d_dev, const float *homo_dev,
    float scale0, float scale1, const SageCamera *cam, float eps, float loss_param, float weight,
    int N, int CS);

/* df::geometric_error_calculate<CS> (geometric_factor_kernels.h:18-24, .cpp:837-880) */
int sage_geometric_error_calculate(
    SageWorkspace *ws, float *error_host, float *num_inliers_host,
    const float *R10_dev, const float *t10_dev,
    const float *bias0_dev, const float *basis0_dev, const float *code0_dev,
    const float *dpt1_dev, const float *mask1_dev, const int32_t *loc1d_dev, const float *homo_dev,
    float scale0, const SageCamera *cam, float eps, float loss_param, float weight, int N, int CS);

/* ---- input producers ---- */
/* UpdateDepth + ComputeSpatialGrad (core/mapping/mapping_utils.h:215-252; caller side of the geometric
 * factor, geometric_factor.cpp:317-347): dpt[H,W] = scale*(bias+basis*code), grad[2,H,W] = scale*centraldiff.
 * The producers are ASYNCHRONOUS on the workspace's stream (unlike the operator calls, which end in a stream
 * synchronise): every device input -- code_dev included -- must stay valid until the stream has passed the call. */
int sage_depth_and_grad(SageWorkspace *ws, float *dpt_dev, float *dpt_grad_dev,
                        const float *bias_dev, const float *basis_dev, const float *code_dev,
                        float scale, int H, int W, int CS);
/* GenerateGaussianPyramidWithGrad (core/mapping/mapper.cpp:1384-1426): feat [FS,H,W], mask [H,W]
 * -> pyr [FS,P], grad [2,FS,P]. */
int sage_gaussian_pyramid_with_grad(SageWorkspace *ws, float *pyr_dev, float *grad_dev,
                                    const float *feat_dev, const float *mask_dev,
                                    const SagePyramid *pyr, int FS);

/* =====================================================================
 * Host-side helpers (pure CPU, no device needed)
 * ===================================================================== */
/* Bind the CALLING thread to the CPUs of the NUMA node the HIP device hangs off (sysfs local_cpulist of its PCI
 * function), intersected with the thread's current affinity mask.  The hybrid window solve reads 3 MB of freshly DMA'd
 * normal equations per LM iteration and the pinned buffers live on the device's node: from the far socket of a
 * two-socket host the iteration is ~10 % slower.  Opt-in (one process per GPU: call it once from the thread that
 * drives the window); returns the number of CPUs bound to, 0 if the topology is not exposed, < 0 on error.
 * r05: the call also watches the host's load for 250 ms (/proc/stat) and keeps to physical cores that are quiet on all their
 * hardware threads -- alone on the NUMA node it narrows the thread's mask to the L3 domain with the most of them -- and the
 * solve's helper threads are placed on quiet cores only (SAGE_BIND_NO_PROBE=1: the plain NUMA-node binding). */
int sage_bind_thread_to_device(int device);
/* Diagnostics of the hybrid solve's thread placement: the CPUs its (up to three) helper threads are pinned to (-1: not
 * placed yet; returns how many entries were written), and how often the placement monitor has moved a helper off a core
 * that another process crowded.
 * r06: the placement monitor -- a background thread that looks at the helpers' run-queue delay and at the load on their
 * cores' other hardware threads every 250 ms and re-pins a crowded helper -- is OPT-IN: SAGE_PLACEMENT_MONITOR=1 in the
 * environment or sage_placement_monitor(1) before the first solve (sage_placement_monitor(0) stops and joins it).  A
 * drop-in library does not edit thread affinities from the background unless asked to. */
int sage_solver_helper_cpus(int *cpus, int n);
int sage_solver_placement_moves(void);
int sage_placement_monitor(int enable);
/* Host threads of the library (r06).  The window solve runs on up to 3 helper threads (+ up to 10 pool workers for
 * loop-closure plans, + the opt-in monitor).  They are started by the first solve that wants them and are JOINABLE:
 * the last sage_window_destroy of the process, sage_shutdown() and process exit (atexit) stop and join them -- nothing
 * is detached, no thread of this library outlives its last window.  sage_shutdown() may be called at any time no
 * solve is in flight (e.g. before dlclose); a later solve starts the threads again.
 * sage_host_threads_running() = how many of them are alive (diagnostic). */
void sage_shutdown(void);
int sage_host_threads_running(void);

/* se3_exp (core/mapping/mapping_utils.h:316-346): R[9], t[3] from omega[3], v[3].  (The void helpers -- this one,
 * sage_pose_retract, sage_lm_config_default -- treat a null argument as a no-op; every int entry point answers a null /
 * out-of-range argument with a status code: tests/test_host_logic.py calls all of them with NULL / 0.) */
void sage_se3_exp(const float *omega, const float *v, float *R, float *t);
/* left retraction T <- exp([v,w]) T (core/gtsam/gtsam_traits.h:45-70; camera_tracker.cpp:491-512);
 * pose/out are 12 floats (R then t), delta = [v(3), w(3)]. */
void sage_pose_retract(const float *pose, const float *delta6, float *out);
/* Higham nearest-PSD of a symmetric-ish n x n matrix in double (the algorithm
 * core/mapping/mapping_utils.h:104-128 intends; see DESIGN.md for the reference's V^T S V slip). */
int sage_nearest_psd(const double *M, int n, double *out);
/* NearestPsd AS THE REFERENCE WROTE IT (mapping_utils.h:104-128): H = V^T diag(sigma) V with the V of Eigen 3.3.9's
 * two-sided Jacobi SVD (its rotation sequence is restated, because the expression depends on V's sign and order
 * conventions), then the LDLT / minimum-eigenvalue bump loop.  Reproduces the reference (fixtures generated with the
 * vendored Eigen) wherever the reference itself is reproducible: see DESIGN.md s6 -- on the gauge-deficient systems
 * the dense factors actually produce, a 1e-15 relative change of the input moves the reference's result by 20 %. */
int sage_nearest_psd_reference(const double *M, int n, double *out);
/* a6 / a7: the HessianFactor blocks of one per-edge system, as PhotometricFactor::linearize
 * (core/gtsam/photometric_factor.cpp:142-218: keys {p0, p1, c0, s0}, block sizes {6, 6, CS, 1}) and
 * GeometricFactor::linearize (core/gtsam/geometric_factor.cpp:120-218: keys {p0, p1, c0, c1, s0, s1}, sizes
 * {6, 6, CS, CS, 1, 1}) cut them: AtA (fp32, row-major D x D, HOST) is widened to double, passed through NearestPsd
 * (psd_mode 0: none, 1: sage_nearest_psd, 2: sage_nearest_psd_reference = as the reference wrote it) and split into
 * the upper-triangular blocks G_ij, i <= j, in the order the reference pushes them (G11 G12 .. G1n G22 ..), each
 * block row-major, concatenated in G_out (sage_factor_block_count doubles); g_out receives Atb widened (D doubles: the
 * g_i are its consecutive segments).  type 0 = photometric (D = 13 + CS), 1 = geometric (D = 14 + 2 CS).
 * dims_out (optional, 6 ints) receives the key dimensions, *nkeys_out their number. */
int sage_factor_block_count(int type, int CS);
int sage_factor_hessian_blocks(int type, int CS, const float *AtA_host, const float *Atb_host, int psd_mode,
                               double *G_out, double *g_out, int32_t *dims_out, int32_t *nkeys_out);
/* solve (A + damp*diag(A)) x = b, column-pivoted Householder QR in fp32 (camera_tracker.cpp:1182-1183). */
int sage_damped_solve_qr_f32(const float *A, const float *b, int n, float damp, float *x);

/* damped solve of the block-sparse normal equations in double (block Cholesky, B <= 40):
 *   (H + diag_add + damp*diag(H + diag_add)) delta = g + g_add
 * packed = [diag K*B*B | link nlinks*B*B (rows = links[2l], cols = links[2l+1], links[2l] < links[2l+1]) | g K*B | 4]
 * (host memory, the layout of sage_window_packed_dev); diag_add / g_add (K*B doubles, may be NULL) carry the
 * diagonal priors.  Returns SAGE_E_NOT_PSD if the damped matrix is not positive definite,
 * SAGE_E_UNSUPPORTED for B > 40. */
int sage_block_solve(const double *packed_host, int K, int nlinks, const int32_t *links, int B, double damp,
                     const double *diag_add, const double *g_add, double *delta);
/* diagnostics: how many half-factorisations of split windows ran as two stages (a look-ahead thread + the chain
 * through the previous row) in this process so far; the factor is the same bit for bit either way. */
long long sage_solve_lookahead_count(void);

/* ---- tracker LM (core/system/camera_tracker.cpp:1034-1310 / 1312-1672) ---- */
typedef struct SageLmConfig
{
  int max_num_iters;         /* tracking_max_num_iters       = 40   */
  float min_grad_thresh;     /* tracking_min_grad_thresh     = 1e-4 */
  float min_param_inc_thresh;/* tracking_min_param_inc_thresh= 1e-2 */
  float init_damp;           /* tracking_init_damp           = 1e-4 */
  float min_damp, max_damp;  /* tracking_min_max_damp        = 1e-6, 1e-2 */
  float damp_dec_factor;     /* tracking_damp_dec_inc_factor = 10, 100 */
  float damp_inc_factor;
  float jac_update_err_inc_threshold; /* 1e-2 */
  int max_inner_evals;       /* window LM only: cap on candidate evaluations per iteration (0 = reference policy: retry until accepted or max_damp) */
  float no_overlap_error;    /* tracker LM: > 0 -> stop with SAGE_E_NO_OVERLAP once the error at the current estimate is >= this
                              * (TrackFrame without the match-geometry term: 9.9 * sum(photo weights), camera_tracker.cpp:1515); 0 = off */
  int linearize_at_candidate;/* window LM only (sage_window_lm_step).  1: the candidate is evaluated by the LINEARIZE
                              * kernels (error and normal equations from one pass, the system at the current estimate kept
                              * aside): an accepted iteration costs one linearize + one solve and no separate error pass, a
                              * rejected one costs a linearize instead of an error pass.  Same accept / reject rule and the
                              * same iterates as the classic sequence (the two kernels' errors agree to fp32 rounding).
                              * sage_window_get_edge then returns the per-edge results of the LAST evaluation (the
                              * candidate's after a rejected one); the packed system is always the current estimate's.
                              * 0 (default) = automatic: this sequence for windows that are reduced over ranks (one
                              * collective per iteration instead of two and no error pass on the shard's critical path),
                              * the classic sequence on a single rank.  -1: the classic sequence always. */
} SageLmConfig;
void sage_lm_config_default(SageLmConfig *cfg);

/* evaluation back-end of the tracker LM: the product wires these to the HIP kernels above; tests may
 * wire them to anything.  Return 0 on success. */
typedef int (*SageTrackLinearizeFn)(void *ctx, const float *pose12, float scale, float *AtA, float *Atb, float *error);
typedef int (*SageTrackErrorFn)(void *ctx, const float *pose12, float scale, float *error);

typedef struct SageLmTraceEntry
{
  float damp, error, candidate_error;
  int accepted, relinearized;
} SageLmTraceEntry;

/* dof = 6 (TrackNewFrame) or 7 (TrackFrame, + scale).  pose12/scale are in/out.  trace (optional) receives
 * up to trace_cap entries, *trace_len the number written. */
int sage_track_lm(const SageLmConfig *cfg, int dof, SageTrackLinearizeFn lin, SageTrackErrorFn err, void *ctx,
                  float *pose12, float *scale, float *final_error, int *iters,
                  SageLmTraceEntry *trace, int trace_cap, int *trace_len);

/* B runs of the same policy in lock-step (the loop detector tracks every surviving candidate against the query keyframe:
 * loop_detector.cpp:165, :321).  sage_track_lm and this call drive ONE definition of the policy (a resumable stepper); per
 * problem the outputs are those of sage_track_lm with callbacks that return the same values.
 * A round: every problem that is not done asks for exactly one evaluation -- the linearisation (want_jac 1: AtA dof x dof
 * row-major at stride 49, Atb at stride 7, error) or the error alone (want_jac 0) at (pose12, scale) -- and `eval` is called
 * once with all n of them, `problem` ascending.  It is not called for a round without requests; a problem that finishes
 * drops out; the call returns when all are done.  A non-zero return of `eval` ends the call with that code (no output is
 * written then).  pose12 [B][12] and scale [B] are in / out; final_error, iters, trace_len ([B], optional); status [B]:
 * SAGE_OK or SAGE_E_NO_OVERLAP; trace (optional) [B][trace_cap].
 * SAGE_E_INVALID for NULL cfg / eval / pose12 / status, dof not 6 or 7, dof 7 with NULL scale, B < 0 or
 * B > SAGE_TRACK_MAX_BATCH (32, defined next to SAGE_MATCH_MAX_BATCH).  B = 0: SAGE_OK, nothing is called. */
typedef int (*SageTrackBatchEvalFn)(void *ctx, int n, const int32_t *problem, const int32_t *want_jac, const float *pose12,
                                    const float *scale, float *AtA, float *Atb, float *error);
int sage_track_lm_batch(const SageLmConfig *cfg, int dof, int B, SageTrackBatchEvalFn eval, void *ctx, float *pose12,
                        float *scale, float *final_error, int *iters, int *status, SageLmTraceEntry *trace, int trace_cap,
                        int *trace_len);

/* product wiring of the two callbacks to the HIP kernels: CameraTracker::TrackNewFrame (dof 6) / TrackFrame (dof 7)
 * with the reference's term composition (camera_tracker.cpp:220-374):
 *   dof 6: error / AtA / Atb = photometric (tracker_photo_*)            [use_photo]
 *                            + reprojection (tracker_reproj_*)           [use_keypoints]      (:282-328, :220-248)
 *   dof 7: photometric with scale (tracker_photo_*_with_scale)          [use_photo]
 *                            + match geometry with scale                 [use_keypoints]      (:330-374, :250-280)
 * dof 7 hands over UNSCALED depths (dpt_map_0 / dpt_scale_0, camera_tracker.cpp:1397,1418): every Jacobian and every
 * candidate evaluation multiplies them by the scale being evaluated (guess_scale_0 * unscaled_*_dpts_0, :264,:273,:431,
 * :453) -- the 7th variable moves the depths, not only the Jacobian column.  dof 6 hands over metric depths.
 * The sums are fp32, term by term, like the reference's `AtA += photo_AtA` on fp32 tensors. */
typedef struct SageTrackProblem
{
  SageWorkspace *ws;
  /* photometric term */
  int32_t use_photo;
  const float *mask1_dev, *dpts0_dev, *homo_dev, *feat0s_dev, *feat1_dev, *grad1_dev;
  const float *weights_dev;
  SagePyramid pyr;
  float eps;
  int32_t N, FS;
  /* keypoint term: NK matched keypoints of frame 0 (depths: metric for dof 6, unscaled for dof 7) */
  int32_t use_keypoints, NK;
  const float *kp_dpts0_dev;          /* [NK]   */
  const float *kp_homo0_dev;          /* [NK,3] */
  const float *kp_matched_2d_dev;     /* dof 6: [NK,2] matched pixel locations in frame 1 (reprojection)       */
  const float *kp_matched_dpts1_dev;  /* dof 7: [NK]   depths of the matched points in frame 1 (match geometry) */
  const float *kp_matched_homo1_dev;  /* dof 7: [NK,3] */
  float kp_loss_param;                /* reproj_loss_param_ / match_geom_loss_param                              */
  float kp_weight;                    /* inlier_multiplier_ * {reproj,match_geom}_factor_weight                  */
} SageTrackProblem;
/* Returns SAGE_OK, or SAGE_E_NO_OVERLAP when TrackFrame's zero-overlap exit fires (cfg->no_overlap_error).  trace
 * (optional) as in sage_track_lm. */
int sage_track_frame(const SageLmConfig *cfg, int dof, const SageTrackProblem *prob,
                     float *pose12, float *scale, float *final_error, int *iters,
                     SageLmTraceEntry *trace, int trace_cap, int *trace_len);
/* B problems tracked in lock-step: sage_track_lm_batch wired to batched kernels.  Per round (one evaluation of every problem
 * that is not done): (dof 7) one scale pass that forms scale * unscaled depths for every problem and term of the round, at
 * most two photometric launches (linearize, error-only: different kernels) over a flattened list of (problem, 256-pixel
 * tile) items with a finalize each, at most two keypoint launches (a workgroup per problem), one ticket and one wait --
 * whatever B.  A problem whose keypoint rows do not fit one workgroup's LDS (the single call's own test: NK > 571 at dof 7,
 * NK > 927 at dof 6) goes through the single call's launches inside the round.
 * CONTRACT: for every b, pose12[b], scale[b], final_error[b], iters[b], status[b] and the trace are byte-identical to
 * sage_track_frame(cfg, dof, &probs[b], ...) on the same workspace and inputs, for every B, every order of the problems and
 * whatever the other problems of the batch do (the per-pixel body and the keypoint contraction are the single call's code;
 * per-tile partials are summed in tile order by one workgroup per problem).
 * probs [B]; pose12 [B][12], scale [B] in / out; final_error, iters, trace_len [B] (optional); status [B]: SAGE_OK or
 * SAGE_E_NO_OVERLAP per problem; trace (optional) [B][trace_cap].
 * SAGE_E_INVALID before any launch: what sage_track_lm_batch and sage_track_frame refuse (per problem), NULL probs with
 * B > 0, and problems that do not share ws, FS, use_photo, use_keypoints, eps and a pyr with equal levels and cameras.
 * B = 0: SAGE_OK, nothing launched. */
int sage_track_frame_batch(const SageLmConfig *cfg, int dof, const SageTrackProblem *probs, int B, float *pose12,
                           float *scale, float *final_error, int *iters, int *status, SageLmTraceEntry *trace,
                           int trace_cap, int *trace_len);

/* ---- overlap statistics of a tracked pose: CameraTracker::ComputeAreaInlierRatio (camera_tracker.cpp:95-169), what
 *      TrackNewFrame (:1289) and TrackFrame (:1644) hand back besides the pose and what NewKeyframeRequired
 *      (deepfactors.cpp:2028-2049) and the loop detector (loop_detector.cpp:130, 173-181, 276-339) decide from ----
 * Over ALL M valid pixels of the keyframe (not the N sampled ones), per point i, in fp32 like the reference:
 *   X = (depth_scale * d_i) * (R * h_i) + t,  pos = X.z > eps           (GenerateReproj2DLocationsNoClamp, mapping_utils.h:671-711)
 *   x1 = X.x / X.z * fx + cx, y1 likewise (no clamping);  x0 = h_i.x * fx + cx, y0 likewise
 *   mask tap = grid_sample(nearest, zeros, align_corners = true) at 2 * x1 / w - 1:  ix = nearbyint(((2 * x1 / w - 1) + 1) / 2 *
 *   (w - 1)), half to even, iy likewise with h (the (w - 1) / w squeeze is the reference's); outside the image or not finite reads 0
 *   in = pos && mask[iy, ix] > 0.5
 * input_area = area of the convex hull of all M (x0, y0); warp_area = that of the (x1, y1) of the `in` points (0 with fewer
 * than three distinct ones);  area_ratio = warp_area / input_area -- 0 / 0 is NaN, as in the reference (all points on one
 * line: both areas 0);  inlier_ratio = n_in_mask / M;  average_motion = mean over `pos` of |(x1, y1) - (x0, y0)| / sqrt(w^2 +
 * h^2) -- NaN without a `pos` point (torch's mean of an empty tensor).
 * The device discards the points strictly inside a polygon of extreme points of their set (they cannot be hull vertices)
 * and hands the host the rest: n_candidates, at most M per set.  Two calls on the same inputs return identical bytes. */
typedef struct SageOverlapStats
{
  double input_area, warp_area;                   /* the two hull areas, px^2 */
  float area_ratio, inlier_ratio, average_motion; /* the reference's three outputs */
  int32_t n_points, n_pos_depth, n_in_mask;       /* M, |z1 > eps|, |mask & z1 > eps| */
  int32_t n_candidates[2];                        /* points that reached the host hull: [input set, warped set] */
} SageOverlapStats;
/* R, t: HOST (row-major R10, t10).  dpts0_dev [M], homo_dev [M,3], mask_dev [h,w] of `cam`: device.  depth_scale multiplies
 * every depth first (1 for TrackNewFrame; guess_scale / dpt_scale_0 for TrackFrame, camera_tracker.cpp:1644).
 * SAGE_E_INVALID (nothing is launched) for a NULL pointer, M <= 0, fx / fy not finite or not positive, w / h < 1.
 * One wait on the workspace's ticket; no blocking copy. */
int sage_track_overlap(SageWorkspace *ws, const float *R, const float *t, const float *dpts0_dev, float depth_scale,
                       const float *homo_dev, int M, const SageCamera *cam, const float *mask_dev, float eps,
                       SageOverlapStats *out);
/* sage_track_overlap for B poses over ONE point set, camera and mask -- the tracked candidates of one loop query
 * (loop_detector.cpp:165-183, :321-342 call ComputeAreaInlierRatio once per candidate).  Row b of `out` equals, byte for
 * byte, what sage_track_overlap(ws, poses[b].R, poses[b].t, dpts0_dev, poses[b].depth_scale, homo_dev, M, cam, mask_dev, eps, .)
 * returns, n_candidates included: a row keeps the single call's partition (min(ceil(M / 256), 32) workgroups, grid-strided),
 * its sums in workgroup order and its device functions.
 * Three launches whatever B (the row is a grid axis), one wait on the workspace's ticket, no blocking copy; the poses travel
 * in the kernel arguments.  The input set does not depend on the pose: its extremes, filter pass and pinned copy happen
 * once (row 0's workgroups), the host hulls it once and writes input_area and n_candidates[0] into every row -- B + 1 host
 * hulls per call where B single calls make 2 B.
 * Memory, shared with sage_track_overlap and kept by the workspace: device 12816 * B + 8 * M * (B + 1) bytes (per row the 32
 * workgroups' partial records: 8 + 8 + 384 bytes each, and 16 bytes of append counters; then the survivors of the input
 * set and of the B warped sets), pinned 32 * B + 8 * M * (B + 1) bytes (the rows' headers, then the same B + 1 sets).
 * SAGE_E_INVALID, before anything touches the device: NULL ws; B < 0 or B > SAGE_OVERLAP_MAX_BATCH; with B > 0 a NULL
 * pointer, M <= 0, or a camera sage_track_overlap refuses.  B = 0: SAGE_OK, nothing is read, launched or waited for.  On
 * an error no row of `out` is meaningful. */
#define SAGE_OVERLAP_MAX_BATCH 32 /* = SAGE_TRACK_MAX_BATCH */
typedef struct SageOverlapPose /* host; row-major R10, t10 */
{
  float R[9], t[3];
  float depth_scale;
} SageOverlapPose;
int sage_track_overlap_batch(SageWorkspace *ws, const SageOverlapPose *poses, int B, const float *dpts0_dev,
                             const float *homo_dev, int M, const SageCamera *cam, const float *mask_dev, float eps,
                             SageOverlapStats *out /* [B] */);
/* Host only, no device: what a batch of B poses over M points reserves (the formulas above; 0 for B = 0) and launches (3; 0
 * for B = 0), and the workgroups of one row.  Every output pointer may be NULL.  SAGE_E_INVALID for B out of range, or
 * M <= 0 with B > 0. */
int sage_track_overlap_batch_plan(int M, int B, int64_t *device_bytes, int64_t *pinned_bytes, int32_t *launches,
                                  int32_t *workgroups_per_row);
/* kernel launches of the workspace's last sage_track_overlap_batch (0: none yet, B = 0, or NULL ws) */
int sage_track_overlap_batch_launches(const SageWorkspace *ws);
/* Stateless host math: area of the convex hull of n 2-D points (xy interleaved, [n,2]) in double arithmetic; 0 for fewer
 * than three distinct points or a collinear set.  The points are ordered first: any permutation of a set gives the
 * identical double.  Points with a non-finite coordinate are left out.  n_vertices (optional): corners of the hull,
 * collinear boundary points not counted (0 when the area is 0).  SAGE_E_INVALID for a NULL `area`, n < 0, or NULL xy with n > 0. */
int sage_convex_hull_area(const float *xy, int n, double *area, int *n_vertices);

/* ---- the mapper's depth-scale correction: Mapper::CorrectDepthScale (mapper.cpp:237-309, every new keyframe) and the loop
 *      detector's df::CorrectDepthScale (mapping_utils.h:797-865, every accepted global loop: its result is the query
 *      scale of the loop-closure pose-scale graph); sage_median_f32 is the torch::median Mapper::InitOneFrame normalises
 *      the first keyframe by (mapper.cpp:181-185) ----
 * Over all M valid pixels of keyframe 0 (the reference keyframe), per point i, in fp32 like the reference:
 *   X = d_i * (R10 * h_i) + t10,  pos = X.z > eps,  x = X.x / X.z * fx + cx, y likewise
 *   grid coordinate gx = (x + 0.5) * (2 / w) - 1, un-normalised by grid_sample (align_corners = false): ix = ((gx + 1) * W - 1) / 2
 *   D1 = bilinear tap of bias1 at (ix, iy), zeros outside, taps summed nw, ne, sw, se (an in-bounds NaN texel gives NaN
 *        whatever its weight);  m = nearest tap of the mask at (nearbyint(ix), nearbyint(iy)), half to even, 0 outside
 *   valid = m * pos,  selected = valid > 0.5,  ratio_i = (X.z * valid) / D1   (inf for D1 == 0 is a value and sorts last)
 * ratio = the LOWER median (element (n_used - 1) / 2 of the sorted values) of the selected ratios, found by an exact radix
 * selection on the device: no sort, nothing of size M crosses PCIe.  Two calls on the same inputs return identical bytes. */
typedef struct SageDepthScaleStats
{
  float ratio;          /* the reference's return value; NaN when n_used == 0, and when !drop_nan and n_nan > 0 */
  int32_t n_points;     /* M */
  int32_t n_pos_depth;  /* |X.z > eps| */
  int32_t n_selected;   /* |valid > 0.5| */
  int32_t n_nan;        /* NaN ratios among the selected */
  int32_t n_used;       /* values the median ran over: n_selected, minus n_nan when drop_nan */
} SageDepthScaleStats;
/* R10, t10: HOST (row-major).
 * dpt0_dev: keyframe 0's depth map [h*w], read at loc1d0_dev [M] (int64, the reference's valid_locations_1d; a location
 *           outside the map reads NaN: the point is not selected), or, with loc1d0_dev == NULL, the M depths already gathered.
 * homo0_dev [M,3]; bias1_dev [h,w]: dpt_map_bias of the keyframe to scale (the BIAS, not its depth map: mapper.cpp:286);
 * mask_dev [h,w]; cam: level 0.
 * drop_nan = 0: Mapper::CorrectDepthScale (a NaN among the selected ratios makes the result NaN, as torch::median does).
 * drop_nan = 1: df::CorrectDepthScale of the loop detector (NaN ratios are removed first, mapping_utils.h:857).
 * ratios_out_dev [M] float, selected_out_dev [M] int32: optional device outputs, the per-point ratio and whether it was selected.
 * SAGE_E_INVALID (nothing is launched) for a NULL required pointer, M <= 0, fx / fy not finite or not positive, w / h < 1.
 * n_used == 0 (e.g. everything behind the camera) is no error: ratio = NaN, SAGE_OK.  One wait on the workspace's ticket. */
int sage_depth_scale_ratio(SageWorkspace *ws, const float *R10, const float *t10, const float *dpt0_dev,
                           const int64_t *loc1d0_dev, const float *homo0_dev, int M, const SageCamera *cam,
                           const float *bias1_dev, const float *mask_dev, float eps, int drop_nan,
                           float *ratios_out_dev, int32_t *selected_out_dev, SageDepthScaleStats *out);
/* torch::median of n device floats (values_dev[loc1d_dev[i]] when loc1d_dev != NULL: mapper.cpp:182): the LOWER median,
 * element (n_used - 1) / 2 of the sorted values (-0 before +0); NaN when a NaN is present and !drop_nan, and when
 * n_used == 0.  Every location must lie inside values_dev (it is not checked).  n_used_host, n_nan_host: optional.  SAGE_E_INVALID (nothing is launched) for a NULL ws, values_dev or
 * median_host, and n <= 0. */
int sage_median_f32(SageWorkspace *ws, const float *values_dev, const int64_t *loc1d_dev, int n, int drop_nan,
                    float *median_host, int *n_used_host, int *n_nan_host);

/* sage_depth_scale_ratio_batch: B reference keyframes warped into ONE keyframe to scale -- the loop detector's case, one
 * query keyframe and every accepted candidate (loop_detector.cpp:194 inside the loop of :143).  The rows differ in pose,
 * point set and M; the bias, the mask and the camera of the keyframe to scale are shared.
 * CONTRACT: out[b], and row b's optional per-point outputs, are byte-identical to sage_depth_scale_ratio on that row's
 * inputs, whatever the other rows, their order and their sizes: the per-point arithmetic is the single call's device
 * function and the selection only sums integers.  A row that selects nothing is no error (ratio NaN) and does not disturb
 * its neighbours.
 * Launches: 5 whatever B and the M_b (sage_depth_scale_ratio_batch_launches) -- the per-point kernel, two digit passes and
 * the finish, each over a flat list of (row, workgroup) items, min(ceil(M_b / 256), 256) of them for row b as in the single
 * call, then the ticket; one wait.  The rows' table travels as a kernel argument: no copy, no per-row launch or memset.
 * (B = 1 runs the single call's kernels: the same five launches.)
 * Memory, shared with the single calls and kept by the workspace: device 4 * sum(M_b) + 24608 * B bytes (the keys of all
 * rows at row offsets; per row three histograms, the counters and the pass state), pinned 32 * B bytes (a record per row).
 * Single and batched calls may be interleaved on one workspace in any order.
 * SAGE_E_INVALID, before anything is launched: a NULL ws, rows, cam, bias1_dev, mask_dev or out; B < 0 or
 * B > SAGE_DEPTH_SCALE_MAX_BATCH; a row with M <= 0 or a NULL dpt0_dev or homo0_dev; a camera sage_depth_scale_ratio
 * refuses.  B = 0: SAGE_OK, nothing is launched. */
#define SAGE_DEPTH_SCALE_MAX_BATCH 32 /* = SAGE_TRACK_MAX_BATCH */
typedef struct SageDepthScaleRow /* one reference keyframe warped into the keyframe to scale */
{
  float R10[9], t10[3];         /* host values, row-major */
  const float *dpt0_dev;        /* as in sage_depth_scale_ratio */
  const int64_t *loc1d0_dev;    /* or NULL: dpt0_dev holds the M gathered depths */
  const float *homo0_dev;       /* [M,3] */
  int32_t M;
  float *ratios_out_dev;        /* optional [M] */
  int32_t *selected_out_dev;    /* optional [M] */
} SageDepthScaleRow;
int sage_depth_scale_ratio_batch(SageWorkspace *ws, const SageDepthScaleRow *rows, int B, const SageCamera *cam,
                                 const float *bias1_dev, const float *mask_dev, float eps, int drop_nan,
                                 SageDepthScaleStats *out /* [B] */);
/* B medians in the same 5 launches: element b equals sage_median_f32(values_dev[b], loc1d_dev ? loc1d_dev[b] : NULL, n[b]),
 * byte for byte.  loc1d_dev may be NULL, and so may any of its entries.  n_used_host, n_nan_host [B]: optional.
 * SAGE_E_INVALID (nothing is launched) for a NULL ws; B out of range; with B > 0 a NULL values_dev, n or median_host, a NULL
 * entry of values_dev, n[b] <= 0.  B = 0: SAGE_OK, nothing is launched. */
int sage_median_f32_batch(SageWorkspace *ws, const float *const *values_dev, const int64_t *const *loc1d_dev,
                          const int32_t *n, int B, int drop_nan, float *median_host, int32_t *n_used_host,
                          int32_t *n_nan_host);
/* Host only, no device: what a batch of B rows of M[b] points reserves (the formulas above), launches (5; 0 for B = 0) and
 * the workgroups of its flat list.  Every output pointer may be NULL.  SAGE_E_INVALID for B out of range, a NULL M with
 * B > 0, or a row with M <= 0. */
int sage_depth_scale_ratio_batch_plan(const int32_t *M, int B, int64_t *device_bytes, int64_t *pinned_bytes,
                                      int32_t *launches, int32_t *workgroups);
/* kernel launches of the workspace's last sage_depth_scale_ratio_batch or sage_median_f32_batch (0: none yet, B = 0, or
 * NULL ws) */
int sage_depth_scale_ratio_batch_launches(const SageWorkspace *ws);

/* ---- the loop detector's bag of words: LoopDetector::AddKeyframe (core/system/loop_detector.cpp:20-42) turns the
 *      descriptors of all valid pixels of a new keyframe into a DBoW2 bag-of-words vector, DetectLoop (:53-111) scores it
 *      against the temporal neighbours and queries the database with it ----
 * Vocabulary (TemplatedTensorVocabulary::load, core/system/tensor_vocabulary.cpp:49-128): node 0 is the root; every other
 * node has a parent, a C-float descriptor and a double weight; a node without children is a leaf and carries a word id.
 * Transform of M points (transform / subset_transform, tensor_vocabulary.cpp:131-245): every point starts at the root; at a
 * node with children c_0..c_{n-1} it goes to argmin_j d_j, d_j = sum_ch (F[ch,i] - desc[c_j][ch])^2 in fp32 (the
 * difference form), the first smallest wins, a NaN distance counts as smallest and the first NaN wins (torch.argmin), until
 * it stands on a leaf.  Every leaf reached by at least one point, with weight > 0, contributes exactly once
 * v[word] = weight * M -- M the number of ALL points, not of those on the leaf (:204-208 multiplies by features.size(1));
 * a leaf with weight <= 0 contributes nothing.  The vector is then L1-normalised in double the way BowVector::normalize
 * does (thirdparty/DBoW2/src/BowVector.cpp:79-101): |v| summed in ascending word order, then every entry divided.  The
 * values are a function of the SET of leaves reached alone.
 * Score (L1Scoring::score, DBoW2/src/ScoringObject.cpp:23-68): over the words both vectors hold, in ascending word order,
 * s += |v - w| - |v| - |w|; the score is -s / 2.
 * Database (TemplatedDatabase::add, queryL1, DBoW2/include/DBoW2/TemplatedDatabase.h:604-675): entries get zero-based ids
 * in the order they are added; a query accumulates the same three-term value per entry over the query's words in
 * ascending order, skips entries with id >= max_id unless max_id == -1, sorts ascending by the accumulated value, cuts to
 * max_results when max_results > 0 and turns every kept value into -value / 2; entries that share no word with the query do
 * not appear.  The reference's std::sort leaves the order of tied values open: HERE TIES GO BY ASCENDING ENTRY ID.
 * Only L1 scoring is implemented (what the shipped vocabulary uses); the TF and TF_IDF weightings give the same transform,
 * the weights live in the nodes. */
#define SAGE_BOW_L1 0 /* DBoW2::ScoringType, in its order */
#define SAGE_BOW_L2 1
#define SAGE_BOW_CHI_SQUARE 2
#define SAGE_BOW_KL 3
#define SAGE_BOW_BHATTACHARYYA 4
#define SAGE_BOW_DOT_PRODUCT 5
typedef struct SageVocabulary SageVocabulary;   /* immutable after creation: any number of workspaces and host threads may share one */
typedef struct SageBowDatabase SageBowDatabase; /* host only */
typedef struct SageVocabularyDesc /* HOST arrays */
{
  int32_t n_nodes;          /* the root counts */
  int32_t C;                /* floats per descriptor */
  const int32_t *parent;    /* [n_nodes]; parent[0] = -1 */
  const float *descriptors; /* [n_nodes * C]; the root's row is ignored */
  const double *weight;     /* [n_nodes] */
  const int32_t *word_id;   /* [n_nodes]; -1 for an inner node */
  int32_t scoring;          /* SAGE_BOW_* */
} SageVocabularyDesc;
/* A node's children are ordered by ascending node index (the order a DBoW2-built file lists them in).  SAGE_E_INVALID,
 * without touching the device, unless 0 <= parent[i] < i for every i > 0, a node has a word id exactly when it has no
 * children, the word ids are a permutation of 0..n_words-1 and there is at least one word below the root; also for a NULL
 * pointer, C < 1 and a scoring that is no SAGE_BOW_* value.  SAGE_E_UNSUPPORTED for C > 64, a node with more than 64
 * children, a leaf deeper than 8, more than 2^20 words, a scoring other than SAGE_BOW_L1.  Ragged trees are legal: any
 * number of children per node, leaves at different depths (DBoW2's k-means makes them).  The device copy (nodes renumbered
 * breadth-first, descriptor rows padded to 4 floats) lives on the device that is current at creation. */
int sage_vocabulary_create(const SageVocabularyDesc *desc, SageVocabulary **out);
void sage_vocabulary_destroy(SageVocabulary *voc);
int sage_vocabulary_num_nodes(const SageVocabulary *voc);    /* these six: -1 for a NULL vocabulary */
int sage_vocabulary_num_words(const SageVocabulary *voc);
int sage_vocabulary_channels(const SageVocabulary *voc);
int sage_vocabulary_depth(const SageVocabulary *voc);        /* of the deepest leaf; the root is at depth 0 */
int sage_vocabulary_max_fanout(const SageVocabulary *voc);
int sage_vocabulary_staged_nodes(const SageVocabulary *voc); /* nodes of the whole top levels the walk keeps in LDS */
typedef struct SageBowStats
{
  int32_t n_points;          /* M */
  int32_t n_words;           /* entries written to word_ids_host / values_host */
  int32_t n_leaves_hit;      /* leaves reached by at least one point */
  int32_t n_zero_weight;     /* ... of them left out for a weight <= 0 */
  int32_t n_inner_nodes_hit; /* inner nodes at least one point passed, the root among them: the reference evaluates one
                                index / subtract / sum / argmin sequence for each */
} SageBowStats;
/* The bag-of-words vector of M points.  desc_dev [C, P] channel-major (feat_desc reshaped to {C, -1}), read at
 * loc1d_dev [M] (int64, the reference's valid_locations_1d) -- or, with loc1d_dev == NULL, desc_dev is [C, M] with P == M:
 * the descriptors already gathered.  THE LOCATIONS ARE NOT RANGE-CHECKED: every one must lie in [0, P).
 * word_ids_host / values_host [capacity]: the vector, ascending word ids, values L1-normalised (they sum to 1; nothing is
 * written when every leaf reached has weight <= 0: n_words = 0, SAGE_OK).  word_of_point_out_dev [M] int32: optional, the
 * word every point reached.  SAGE_E_INVALID (nothing is launched) for a NULL required pointer, M <= 0, P < 1, P != M without
 * locations, capacity < min(M, n_words of the vocabulary).  One kernel walks the tree (its top levels in LDS), one compacts
 * the words reached into pinned memory: one wait on the workspace's ticket, no blocking copy, nothing of size M crosses
 * PCIe.  Two calls on the same inputs return identical bytes. */
int sage_bow_transform(SageWorkspace *ws, const SageVocabulary *voc, const float *desc_dev, const int64_t *loc1d_dev, int M,
                       int P, int32_t *word_ids_host, double *values_host, int capacity, int32_t *word_of_point_out_dev,
                       SageBowStats *out);
/* L1 score of two vectors (strictly ascending word ids; values finite).  SAGE_E_INVALID otherwise, and for a NULL score or a
 * NULL array with n > 0.  Host only. */
int sage_bow_score(const int32_t *ids1, const double *vals1, int n1, const int32_t *ids2, const double *vals2, int n2,
                   double *score);
/* The database: an inverted file, one row per word.  add and query may be called from several threads (one mutex). */
int sage_bow_db_create(int n_words, SageBowDatabase **out);
void sage_bow_db_destroy(SageBowDatabase *db);
/* -> the new entry's id (>= 0), or SAGE_E_INVALID: ids not strictly ascending or outside [0, n_words), a value that is
 * not finite.  n == 0 adds an entry without words, as the reference does for an empty vector. */
int sage_bow_db_add(SageBowDatabase *db, const int32_t *ids, const double *vals, int n);
int sage_bow_db_size(const SageBowDatabase *db); /* entries; -1 for NULL */
/* entry_ids / scores [capacity]: best first; *n_out: how many there are.  More results than capacity: SAGE_E_INVALID,
 * *n_out tells how many, nothing else is written.  An empty database or an empty query: *n_out = 0, SAGE_OK. */
int sage_bow_db_query(const SageBowDatabase *db, const int32_t *ids, const double *vals, int n, int max_results, int max_id,
                      int32_t *entry_ids, double *scores, int capacity, int *n_out);

/* ---- training the vocabulary: TemplatedVocabulary::create (thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:545-572)
 *      as the reference's voc_builder tool runs it on FTensor descriptors: HKmeansStep (:627-815), initiateClustersKMpp
 *      (:829-909), createWords (:914-934), setNodeWeights (:939-989), with FTensor::meanValue / distance
 *      (core/system/dl_descriptor.cpp:6-28) ----
 * Hierarchical k-means over M training descriptors of C floats, level by level; all nodes of a level in the same launches.
 * A NODE's points are taken in ascending training order (the index into desc_dev's columns).  The root holds all M points
 * and is at level 0; its children are at level 1.
 *   n <= k points (:646-656): one child per point, child j carries point j's descriptor and holds that point alone.
 *   n > k: kmeans++ seeding, then Lloyd rounds t = 1, 2, ...: round 1 assigns to the seeded centres, round t > 1 to the means
 *     of round t-1's clusters.  A point goes to the centre with the smallest d2 = sum_ch (x - c)^2, accumulated in fp32 in
 *     channel order exactly as sage_bow_transform's walk does; the first smallest wins (:719-730; descriptors must be
 *     finite, a NaN is never smaller here).  The node stops at the first round t >= 2 with
 *     (double)((float)mismatch / (float)n) < 1.0e-3, mismatch = the points whose cluster differs from round t-1's (:749-765).
 *     Its children carry the centres that PRODUCED the final assignment (not the means after it) and hold its clusters.
 *     max_iterations > 0: a node that has not stopped at round t = max_iterations stops there all the same, with that
 *     round's centres and assignment, and is counted in SageVocabularyBuildStats::nodes_capped (the reference has no cap;
 *     0 = none; max_iterations = 1 is legal: the seeded centres).
 *   A child with more than one point is split again while its level is < L (:792-813); every other child is a leaf.
 * Distance: d2 above decides every argmin.  Where the reference uses the value of F::distance (the L2 norm, not its square)
 * -- kmeans++'s min_dists, its `> 0` test, dist_sum and the cut (:846-907) -- the value is (double)sqrtf(d2): the seeding is
 * proportional to D, not to D^2, as in the reference.
 * Seeding of a node (positions p = 0..n-1 in its order; u(j) = (double)(draw(j) >> 11) * 2^-53 in [0, 1), draw below):
 *   centre 0 = point min(n - 1, (int64)(u(0) * (double)n))                                       [RandomInt(0, n-1)]
 *   round r = 1..k-1: min_d[p] = dist(p, centre 0) for r = 1; afterwards, where min_d[p] > 0, the smaller of min_d[p] and
 *     dist(p, centre r-1).  dist_sum = the sum of min_d: per TILE (256 consecutive positions of the node, the last one
 *     partial) the fp64 sum of its values by the pairwise tree that adds lanes l and l + s for s = 1, 2, 4, ..., 128
 *     (positions past the node's end count 0), then the tiles' sums added in tile order.  dist_sum == 0 ends the seeding:
 *     the node has r centres (fewer than k children).  Otherwise cut = u(r + a k) * dist_sum for the first a = 0, 1, ...
 *     with cut != 0 (the do-while of :884-887; after a = 63 cut = dist_sum) [RandomValue(0, dist_sum)], and centre r is the
 *     point picked so: the first tile whose running sum S_t = S_{t-1} + (its sum) reaches cut (S_t >= cut); inside it, from
 *     S_{t-1}, min_d is added position by position and the first position whose running sum reaches cut is taken; if none
 *     does (the tree sum and the sequential sum round differently), the tile's last position with min_d > 0.
 * draw(j) of a node = sage_vocabulary_build_draw(seed, path, depth, j): path = the child indices from the root to the node
 *   (depth 0 for the root), with mix(z) = { z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *   z ^ (z >> 31) } and G = 0x9E3779B97F4A7C15 (splitmix64), all in uint64:
 *     h = mix(seed + G); for i < depth: h = mix((h ^ (uint64)path[i]) + G); draw = mix(h + (uint64)(j + 1) * G).
 *   (DBoW2 draws from libc rand() in recursion order; that stream cannot be reproduced by a level-synchronous build.)
 * Centre update -- A DELIBERATE DEVIATION: per cluster and channel the sum of its points in fp64 -- per tile in ascending
 *   position, then the tiles' sums in tile order --, divided by the cluster's size in fp64, rounded once to fp32.  The
 *   reference adds fp32 tensors one by one and divides in fp32 (dl_descriptor.cpp:11-18); its rounding depends on the order
 *   and is further from the exact mean.
 * Emptied cluster -- THE SECOND DEVIATION: a cluster that loses all its points keeps its previous centre (and becomes a
 *   leaf no point reaches).  The reference's meanValue reads descriptors[0] of an empty vector: undefined behaviour.
 * Numbering (DBoW2's creation order): node 0 is the root; a node's children get consecutive ids when the node is finished,
 *   then the children that are split are finished depth-first in child order.  Words are the leaves in ascending node id.
 *   parent[i] < i holds.  With equal draws these are the arrays the reference would write.
 * Weights: TF / BINARY: every word 1.  IDF / TF_IDF: Ni = the training documents with at least one point whose walk through
 *   the finished tree (sage_bow_transform's own kernel) ends on word i; weight = log((double)NDocs / (double)Ni) on the host;
 *   a word no document reaches keeps 0.  (The walk sends a point to the leaf the build holds it in, except duplicates inside
 *   a node of n <= k points, which all walk to the first of them -- as in the reference.)
 * Two builds of the same input give identical bytes: no float atomics, every sum has a fixed order. */
#define SAGE_VOC_TF_IDF 0 /* DBoW2::WeightingType, in its order */
#define SAGE_VOC_TF 1
#define SAGE_VOC_IDF 2
#define SAGE_VOC_BINARY 3
#define SAGE_VOC_BUILD_MAX_LEVELS 8
typedef struct SageVocabularyBuild SageVocabularyBuild;
typedef struct SageVocabularyBuildConfig
{
  int32_t k, L;           /* branching factor, depth levels */
  int32_t weighting;      /* SAGE_VOC_* */
  int32_t scoring;        /* SAGE_BOW_* (recorded in the result; only SAGE_BOW_L1 can be created) */
  int32_t max_iterations; /* Lloyd rounds per node; 0 = no cap */
  uint64_t seed;
} SageVocabularyBuildConfig;
typedef struct SageVocabularyBuildStats
{
  int32_t levels;                                  /* levels that had a node to split (<= L) */
  int32_t n_nodes, n_words;                        /* of the finished tree, the root counted */
  int32_t nodes_capped;                            /* nodes stopped by max_iterations */
  int32_t nodes[SAGE_VOC_BUILD_MAX_LEVELS];        /* [l]: nodes split at level l (the root: l = 0) ... */
  int32_t kmeans_nodes[SAGE_VOC_BUILD_MAX_LEVELS]; /* ... of them with n > k */
  int32_t seed_rounds[SAGE_VOC_BUILD_MAX_LEVELS];  /* seeding rounds run at level l: k - 1, or 0 without a k-means node */
  int32_t rounds[SAGE_VOC_BUILD_MAX_LEVELS];       /* Lloyd rounds run at level l = those of its slowest node */
  int32_t launches[SAGE_VOC_BUILD_MAX_LEVELS];     /* kernel launches of level l */
  int32_t waits[SAGE_VOC_BUILD_MAX_LEVELS];        /* ticket waits of level l */
} SageVocabularyBuildStats;
/* k 10, L 4 (tools/voc_builder.cpp:33-34), SAGE_VOC_TF_IDF, SAGE_BOW_L1, max_iterations 100, seed 0 */
void sage_vocabulary_build_config_default(SageVocabularyBuildConfig *cfg);
/* desc_dev [C, M] channel-major on the device (sage_bow_transform's pre-gathered form); doc_begin_host [n_docs + 1]: document
 * d holds the points doc_begin[d] .. doc_begin[d + 1] - 1; ascending (empty documents are legal), [0] = 0, [n_docs] = M.
 * SAGE_E_INVALID, before anything touches the device: a NULL pointer, k < 2, L < 1, C < 1, M < 1, n_docs < 1, offsets that
 * are not such a sequence, max_iterations < 0, a weighting that is no SAGE_VOC_* or a scoring that is no SAGE_BOW_* value.
 * SAGE_E_UNSUPPORTED: C > 64, k > 64, L > 8, k^L > 2^20, M >= 2^31.
 * Per level: one launch that seeds (centre 0, the n <= k nodes), k - 1 seeding rounds of launches_per_seed_round launches,
 * Lloyd rounds of launches_per_lloyd_round launches and one ticket wait each -- nodes that stopped drop out of the round's
 * work list --, then the level's end (centres and child sizes out, the stable partition of every node's points by child: two
 * launches, a copy, the ticket) and one wait.  Then the leaf of every point, the walk and the document counts.  The launches of a round do not depend on the number of nodes. */
int sage_vocabulary_build(SageWorkspace *ws, const SageVocabularyBuildConfig *cfg, const float *desc_dev, int C, int64_t M,
                          const int64_t *doc_begin_host, int n_docs, SageVocabularyBuild **out);
/* the finished tree, as sage_vocabulary_create takes it; the arrays belong to the build (inner nodes have weight 0) */
int sage_vocabulary_build_desc(const SageVocabularyBuild *build, SageVocabularyDesc *desc);
/* *ni [*n_words] (host, owned by the build): Ni of every word; all 0 under TF / BINARY, where it is not computed */
int sage_vocabulary_build_docs_with_word(const SageVocabularyBuild *build, const int32_t **ni, int *n_words);
/* *leaf_node_dev [M] (device, owned by the build): per training point the node id of the leaf that holds it */
int sage_vocabulary_build_node_of_point(const SageVocabularyBuild *build, const int32_t **leaf_node_dev);
int sage_vocabulary_build_stats(const SageVocabularyBuild *build, SageVocabularyBuildStats *stats);
/* What a build allocates and launches, without a device.  With Cp = 4 ceil(C / 4), W = k^L,
 * A = min(k^(L-1), max(1, M / 2)) (nodes split at one level), T = M / 256 + min(k^(L-1), max(1, M / (k + 1))) (tiles of the
 * k-means nodes of one level), integer divisions:
 *   device_bytes = M (4 Cp + 8 + 4 + 4 + 4 + 4 + 4) + 8 A k Cp + 4 A + T (8 k C + 4 k + 4 k + 4 + 8) + 4 W + 16 + 2^24
 *     (rows | min_d | two orders, cluster, leaf, word of every point | both centre sets | centre counts | per tile: sums,
 *      sizes, offsets, mismatches, seeding sum | Ni | counter | document flags); 8 (n_docs + 1) more for the offsets
 *   pinned_bytes = 32 A + 8 T + 16 A + 4 A k + 4 A k + 4 A k Cp
 *     (node records | work items | round results | picks | child sizes | centres)
 *   launches_per_seed_round = 2, launches_per_lloyd_round = 2.
 * SAGE_E_INVALID / SAGE_E_UNSUPPORTED as sage_vocabulary_build for C, M, k, L; every output pointer may be NULL. */
int sage_vocabulary_build_plan(int C, int64_t M, int k, int L, int64_t *device_bytes, int64_t *pinned_bytes,
                               int32_t *launches_per_seed_round, int32_t *launches_per_lloyd_round);
/* draw j of the node at `path` [depth] (see above); path may be NULL with depth <= 0.  Host only. */
uint64_t sage_vocabulary_build_draw(uint64_t seed, const int32_t *path, int depth, int j);
void sage_vocabulary_build_destroy(SageVocabularyBuild *build);

/* ---- robust registration of keypoint matches: the step between sage_cycle_match and the keypoint factors ----
 * CameraTracker::FeatureMatchingGeo (core/system/camera_tracker.cpp:575-768, :770-947), MatchGeometryFactor's constructor
 * (core/gtsam/match_geometry_factor.cpp:98-190) and the loop-MG factor's gather two 3-D point sets from the cycle-consistent
 * matches, build per-point noise bounds max(mult * d / f, 5e-4), call teaser::RobustRegistrationSolver::solve(src, dst,
 * noise_bounds) and keep getTranslationInliers().  Here: sage_match_points (the gather), sage_robust_registration (the solve
 * in the reference's shipped configuration: inlier_selection_mode none, chain TIMs for the rotation, GNC-TLS,
 * estimate_scaling).  What the solver does there (thirdparty/TEASER-plusplus/teaser/src/registration.cc):
 *   1. every pair i < j, in the order i * N - i (i + 1) / 2 + (j - i - 1), gives a scale measurement in fp64:
 *      v1 = |src_j - src_i|, v2 = |dst_j - dst_i|, X = v2 / v1, r = ((nb_i + nb_j) * sqrt(cbar2)) * (1 / v1), w = 1 / r^2
 *   2. the truncated-least-squares vote (ScalarTLSEstimator::estimate, :21-88): the 2 * pairs interval endpoints X - r
 *      (entering) and X + r (leaving) sorted; running sums of e, e w, e w X, e r, e X, e X^2 (e = +1 / -1) over them; at every
 *      endpoint x = sum wX / sum w and cost = card x^2 + sum X^2 - 2 x sum X + (sum of all r - sum e r); the scale is x at the
 *      first smallest cost.  ON THE DEVICE: a pair kernel, a bitonic sort of (key, payload), a three-phase fp64 scan fused
 *      with the cost and the argmin, a count of the pairs with |X - scale| <= r
 *   3. the rotation: GNC-TLS over the N chain TIMs (:596-657, :990-1101) with svdRot (utils.h:121-136), on the host in fp64
 *   4. the translation: three scalar votes over N values (:361-388) and the AND of their masks, on the host in fp64
 * THE ONE DELIBERATE DIFFERENCE: a pair with v1 == 0 (coincident src points; also a pair whose X or r is not finite, or r <= 0) has no
 * defined behaviour in the reference -- NaN keys go into std::sort.  Here such a pair leaves the vote and is counted in
 * n_degenerate_pairs.  The reference's std::sort leaves the order of tied endpoints open: here ties go by pair, entering
 * first.  The device sums run in a fixed tree order, not sequentially: scale agrees with the sequential sum within the bound
 * of a reordered sum (tests/test_gpu_registration.py), and two calls on the same inputs return identical bytes.
 * Workspace bytes (device, kept by the workspace, grow with N): with pairs = N (N - 1) / 2 and P = the power of two
 * >= max(2 * pairs, 4096):  12 P (keys 8, payloads 4) + 16 pairs (X, r) + 160 (P / 2048) + 80 (per-tile sums,
 * offsets and minima, the two counters); N = 512: 5.2 MB, N = 1024: 21 MB.  Pinned: 64 + 32 N. */
#define SAGE_REG_MAX_POINTS 1024 /* 523 776 pairs; 1 047 552 endpoints */
enum { SAGE_REG_CHAIN = 0, SAGE_REG_COMPLETE = 1 };                                                  /* rotation_tim_graph */
enum { SAGE_REG_SELECT_PMC_EXACT = 0, SAGE_REG_SELECT_PMC_HEU = 1, SAGE_REG_SELECT_KCORE_HEU = 2, SAGE_REG_SELECT_NONE = 3 }; /* teaser's order */
enum { SAGE_REG_GNC_TLS = 0, SAGE_REG_FGR = 1 };                                                     /* rotation_algorithm */
typedef struct SageRegistrationParams /* teaser::RobustRegistrationSolver::Params, the fields the shipped path reads */
{
  double noise_bound;              /* scalar bound: only the GNC's mu initialisation reads it (registration.cc:648-650, :1022-1050) */
  double cbar2;                    /* 1 */
  int rotation_max_iterations;     /* 20 */
  double rotation_cost_threshold;  /* 1e-4 */
  double rotation_gnc_factor;      /* 1.4 */
  int rotation_tim_graph;          /* SAGE_REG_CHAIN only; COMPLETE -> SAGE_E_UNSUPPORTED */
  int inlier_selection_mode;       /* SAGE_REG_SELECT_NONE only; the clique modes -> SAGE_E_UNSUPPORTED */
  int rotation_algorithm;          /* SAGE_REG_GNC_TLS only; FGR -> SAGE_E_UNSUPPORTED */
} SageRegistrationParams;
typedef struct SageRegistrationResult /* host */
{
  int valid;                       /* 0: N < 2, or no pair left in the vote (nothing else is meaningful then) */
  double scale, R[9] /* row-major */, t[3];
  int n_inliers;                   /* = getTranslationInliers().size() */
  int n_pairs, n_degenerate_pairs, n_scale_inlier_pairs;
  int rotation_iterations;         /* the GNC's loop index at its exit (0: it left at the mu <= 0 test); max_iterations when it ran out */
  int n_rotation_inliers;          /* chain TIMs with a final weight >= 0.5 */
  double scale_cost;               /* the vote's minimum */
} SageRegistrationResult;
/* src_dev, dst_dev [N][3], noise_bounds_dev [N]: fp32 device arrays (the reference widens fp32 tensors to double before the
 * solve); everything from the pair measurements on is fp64.  inliers_host / inliers_dev [N] (each may be NULL): the
 * translation inliers, ascending; n_inliers entries are written, on return also on the device.  SAGE_E_INVALID (nothing is
 * launched) for a NULL required pointer, N < 0 or N > SAGE_REG_MAX_POINTS, cbar2 / noise_bound / gnc factor not positive and
 * finite (factor <= 1), rotation_max_iterations < 0, a mode that is no SAGE_REG_* value; SAGE_E_UNSUPPORTED for the modes
 * named above.  N < 2: SAGE_OK, valid = 0, n_inliers = 0 (the reference never calls the solver there).  The last kernel
 * publishes scale, the counts and the N points with their bounds into pinned memory and posts the workspace's ticket: one
 * wait, no blocking copy (one more wait when inliers_dev is asked for). */
int sage_robust_registration(SageWorkspace *ws, const float *src_dev, const float *dst_dev, const float *noise_bounds_dev, int N,
                             const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host,
                             int32_t *inliers_dev);
/* host, fp64: ScalarTLSEstimator::estimate as written (a stable sort of the endpoints by value, the sequential sums, the first
 * smallest cost).  estimate, inliers [n] (1: |X - estimate| <= range): each may be NULL.  SAGE_E_INVALID for a NULL X or
 * ranges or n < 1.  Used by the translation step and by tests. */
int sage_tls_estimate(const double *X, const double *ranges, int n, double *estimate, uint8_t *inliers);
/* host, fp64: steps 3 and 4 for a given scale (what sage_robust_registration runs after the device vote; one entry point more
 * than the vote needs: tests and a caller with its own scale use it).  src, dst [N][3], noise_bounds [N]: HOST fp32 arrays,
 * N >= 2.  Fills R, t, n_inliers, rotation_iterations, n_rotation_inliers of *res (scale is stored as given, valid = 1);
 * inliers_host [N] and rotation_mask [N] (1: the chain TIM i -> i + 1 kept its weight) may be NULL. */
int sage_registration_finish(const float *src, const float *dst, const float *noise_bounds, int N, double scale,
                             const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host,
                             uint8_t *rotation_mask);
/* The gather in front of the solver (camera_tracker.cpp:654-714, :849-909; match_geometry_factor.cpp:97-158).  All arrays on
 * the device.  cyc_inlier_flags [K] (from sage_cycle_match), raw_matched_loc1d_1 [K], dpts0 [K] and homo0 [K][3]: per
 * keypoint.  The flagged keypoints are compacted in ascending order (torch::nonzero); per kept keypoint, in fp32 and in the
 * reference's order of operations (true divisions, as torch evaluates them on the CPU):
 *   pts0 = (d0 / depth_divisor0) * homo0;   x = fmod((float)loc, (float)W), y = floor((float)loc / (float)W)
 *   homo1 = ((x - cx) / fx, (y - cy) / fy, 1);   dpts1 = dpt_map_1[loc];   pts1 = dpts1 * homo1
 *   noise_bounds = max((noise_multiplier * d) / ((fx + fy) / 2), 5e-4), d = d0 (noise_from 0) or dpts1 (noise_from 1)
 * kept [K]: the keypoints' positions in 0..K-1.  *M_host: how many were kept (0: nothing else is written);
 * *mean_noise_depth_host (may be NULL): the mean of d, summed in fp64 and rounded once -- NOT pinned to torch::mean's
 * reduction order.  A location outside [0, cam->w * cam->h) reads a NaN depth.  SAGE_E_INVALID for a NULL pointer other than
 * mean_noise_depth_host, K < 1, W < 1, fx / fy not positive and finite, noise_from not 0 or 1.  One kernel, one wait. */
int sage_match_points(SageWorkspace *ws, const int32_t *cyc_inlier_flags, const int64_t *raw_matched_loc1d_1, const float *dpts0,
                      const float *homo0, float depth_divisor0, const float *dpt_map_1, const SageCamera *cam, int K, int W,
                      float noise_multiplier, int noise_from, float *pts0, float *pts1, float *noise_bounds, float *homo1,
                      float *dpts1, int32_t *kept, int *M_host, float *mean_noise_depth_host);

/* ---- B registrations in one call: the scale votes of all of them in one sort ----
 * THE CONTRACT.  Row b of res, of inliers_host (row stride inliers_stride) and of probs[b].inliers_dev holds, byte for byte,
 * what sage_robust_registration writes for problem b alone with p->noise_bound = probs[b].noise_bound (p->noise_bound itself
 * is NOT read) -- whatever else is in the batch, in whatever order, and for every SAGE_REG_SORT_TILE.  Only the first
 * n_inliers entries of an inlier row are written, as there.  sage_match_points_batch gives the same guarantee against
 * sage_match_points (item b's six output arrays, M_host[b], mean_noise_depth_host[b]; M = 0: nothing else is written).
 * Problems that do not vote: N < 2 gets the single call's answer (valid = 0, everything zero), takes no part in any launch
 * and none of its pointers is read; a batch in which nothing votes launches nothing.  A problem whose vote is empty (every
 * pair degenerate) gets valid = 0 with n_pairs and n_degenerate_pairs like the single call; its neighbours are unaffected.
 * Layout: the voting problems are segments of one keys / payload / pairs allocation, ordered by descending P (the power of
 * two >= max(2 pairs, 4096), as the single call chooses it), rows of equal P in the caller's order; the caller's row order
 * never changes.  Every kernel of the vote runs once over (segment, block) items; a sort stage with distance k runs over the
 * segments with P >= k.  LAUNCHES: those of the largest problem alone (sage_robust_registration: its sort's launches + 6) + 1
 * -- the ticket is a launch of its own behind the per-problem publish -- whatever B and the other N; 0 when nothing votes.
 * The one exception: a batch in which ONE problem votes takes sage_robust_registration's own path for it (the batched
 * kernels with one segment measured 0.97 x the single call): its launches exactly, without the + 1.
 * When an inliers_dev row with inliers is asked for: 2 more (one copy kernel over all such rows, one ticket).
 * sage_robust_registration_batch_launches reports what the workspace's last batch spent, sage_robust_registration_batch_plan
 * what a batch of given sizes will spend, without a device.
 * Workspace bytes, with the sums over the voting problems: device Sum (12 P + 16 pairs + 160 (P / 2048) + 80), pinned
 * Sum (64 + 32 N): B = 20 at N = 512: 105.2 MB and 0.33 MB; the cap, 32 x 1024: 673.5 MB and 1.05 MB.  Kept by the workspace.
 * Waits: one for the votes; the finishes (sage_registration_finish, serial, in row order) run on the calling thread; one more
 * wait when an inliers_dev row was written.
 * SAGE_E_INVALID, before anything touches the device: NULL ws, probs, p or res with B > 0; B < 0 or B > SAGE_REG_MAX_BATCH; an
 * N < 0 or > SAGE_REG_MAX_POINTS; for a problem with N >= 2 a NULL src_dev, dst_dev or noise_bounds_dev or a noise_bound that
 * is not positive and finite; inliers_host given with inliers_stride below the largest N; the parameter checks of
 * sage_robust_registration with the same codes (noise_bound apart), SAGE_E_UNSUPPORTED for the modes included.  B = 0:
 * SAGE_OK, nothing is read, checked further or launched. */
#define SAGE_REG_MAX_BATCH 32
typedef struct SageRegistrationProblem /* device pointers; N may differ per problem */
{
  const float *src_dev, *dst_dev, *noise_bounds_dev; /* [N][3], [N][3], [N] */
  int32_t N;                                         /* 0 .. SAGE_REG_MAX_POINTS */
  double noise_bound;                                /* replaces p->noise_bound for this problem */
  int32_t *inliers_dev;                              /* [N] or NULL */
} SageRegistrationProblem;
int sage_robust_registration_batch(SageWorkspace *ws, const SageRegistrationProblem *probs, int B, const SageRegistrationParams *p,
                                   SageRegistrationResult *res /* [B] */, int32_t *inliers_host /* [B][inliers_stride] or NULL */,
                                   int inliers_stride);
/* host only, no device: what a batch of these sizes will do.  N [B]; every output may be NULL.  device_bytes, pinned_bytes:
 * the formulas above; launches: of the votes (at the SAGE_REG_SORT_TILE in effect); order [B]: the rows of the voting
 * problems in the order of their segments, then -1 for every problem that does not vote.  SAGE_E_INVALID for B out of range,
 * NULL N with B > 0, an N out of range. */
int sage_robust_registration_batch_plan(const int32_t *N, int B, int64_t *device_bytes, int64_t *pinned_bytes, int32_t *launches,
                                        int32_t *order /* [B] or NULL */);
/* the kernel launches of the workspace's last sage_robust_registration_batch (0: none yet, nothing voted, or NULL ws); in
 * SAGE_REG_FINISH_DEVICE mode what was really spent: the votes' launches + 1 (the finish), and no row-copy pair */
int sage_robust_registration_batch_launches(const SageWorkspace *ws);

/* ---- the finish of a batch of registrations on the device: steps 3 and 4 in one kernel, one workgroup per problem ----
 * Opt-in per workspace.  SAGE_REG_FINISH_HOST (the default): everything above as written, not a launch or a byte differs.
 * SAGE_REG_FINISH_DEVICE: sage_robust_registration, sage_robust_registration_batch and sage_loop_precheck run
 * reg_finish_kernel behind the vote instead of sage_registration_finish on the calling thread: the chain TIMs, the GNC-TLS
 * rotation (the nine sums of H and the cost as fixed-order trees over 256 lanes, the 3x3 SVD of the host's own source in
 * every lane), the three translation votes (a bitonic sort of the 2 N endpoints in LDS, ties by position as the host's
 * stable sort, then the scale vote's scan and first smallest cost), the AND of the masks and the ascending inlier list,
 * all in fp64.  The kernel writes R, t, the counts and the list into a pinned record of its own (128 + 8 N bytes per voting
 * problem, behind the votes' records) and the list straight into the problem's inliers_dev row (the pre-check's
 * inlier_kp_dev row: through kept); the host reads the records and does no arithmetic.  LAUNCHES: the votes' + 1; the
 * row-copy kernel and its ticket do not run.  Waits: one (the pre-check: three).  LDS: 49 840 bytes per workgroup.
 * THE CONTRACT in DEVICE mode: row b of a batch equals, byte for byte, the single call in DEVICE mode on problem b alone,
 * whatever else is in the batch, in whatever order, for every SAGE_REG_SORT_TILE (the workgroup's size and its reduction
 * trees are functions of N alone); two calls on the same inputs return identical bytes.  Against HOST mode: the counts, the
 * list and rotation_iterations are equal wherever no discrete decision sits within rounding of its threshold; R and t
 * differ by the rounding of reordered sums (tests/test_gpu_registration_finish.py states the bounds).
 * rotation_max_iterations above SAGE_REG_FINISH_MAX_ITERATIONS: SAGE_E_UNSUPPORTED in DEVICE mode, before anything is
 * launched (the kernel's loops are bounded; HOST mode accepts any cap).  Non-finite points: an unspecified answer in bounded
 * time, nothing outside the problem's arrays is touched. */
enum { SAGE_REG_FINISH_HOST = 0, SAGE_REG_FINISH_DEVICE = 1 };
#define SAGE_REG_FINISH_MAX_ITERATIONS 1000 /* the reference ships 20 */
/* SAGE_E_INVALID: NULL ws, a mode that is neither */
int sage_workspace_set_registration_finish(SageWorkspace *ws, int mode);
/* the workspace's mode; SAGE_REG_FINISH_HOST for NULL */
int sage_workspace_registration_finish(const SageWorkspace *ws);
/* steps 3 and 4 for given scales, on the device whatever the workspace's mode: what sage_registration_finish is on the host.
 * probs as in sage_robust_registration_batch (probs[b].noise_bound replaces p->noise_bound; inliers_dev rows are written by
 * the kernel); scales: HOST [B], any value is taken as given (as the host's call does).  A row with N < 2 gets the zeroed
 * result and takes no part.  Fills valid = 1, scale (as given), R, t, n_inliers, rotation_iterations and n_rotation_inliers
 * of res[b]; the vote's fields stay 0.  inliers_host [B][inliers_stride] and rotation_masks [B][inliers_stride] (uint8; 1:
 * the chain TIM i -> i + 1 kept its weight) may be NULL; of a row the first n_inliers resp. N entries are written.  One
 * launch (a workgroup per row with N >= 2) plus the ticket, one wait; nothing is launched when no row has N >= 2.  Pinned:
 * Sum (128 + 8 N).  SAGE_E_INVALID / SAGE_E_UNSUPPORTED, before anything touches the device: as
 * sage_robust_registration_batch (inliers_stride is checked when either host array is given), NULL scales with B > 0, and
 * SAGE_E_UNSUPPORTED for rotation_max_iterations above SAGE_REG_FINISH_MAX_ITERATIONS.  B = 0: SAGE_OK. */
int sage_registration_finish_batch(SageWorkspace *ws, const SageRegistrationProblem *probs, int B, const double *scales /* host [B] */,
                                   const SageRegistrationParams *p, SageRegistrationResult *res /* [B] */,
                                   int32_t *inliers_host /* [B][inliers_stride] or NULL */, int inliers_stride,
                                   uint8_t *rotation_masks /* [B][inliers_stride] or NULL */);
/* host only, no device: what sage_robust_registration_batch will do for these sizes in DEVICE mode (every output may be
 * NULL).  launches: sage_robust_registration_batch_plan's + 1, 0 when nothing votes; pinned_bytes: Sum over the voting
 * problems (64 + 32 N) + (128 + 8 N); lds_bytes: 49 840, the finish kernel's per workgroup (0 when nothing votes);
 * workgroups: of the finish kernel, the voting problems.  SAGE_E_INVALID as sage_robust_registration_batch_plan. */
int sage_registration_finish_plan(const int32_t *N, int B, int32_t *launches, int64_t *pinned_bytes, int32_t *lds_bytes,
                                  int32_t *workgroups);
typedef struct SageMatchPointsItem /* device pointers: one problem's arrays of sage_match_points */
{
  const int32_t *cyc_inlier_flags;     /* [K] */
  const int64_t *raw_matched_loc1d_1;  /* [K] */
  const float *dpts0, *homo0;          /* [K], [K][3] */
  const float *dpt_map_1;              /* [cam->w * cam->h] */
  float *pts0, *pts1, *noise_bounds, *homo1, *dpts1; /* outputs: [K][3], [K][3], [K], [K][3], [K] */
  int32_t *kept;                       /* output [K] */
} SageMatchPointsItem;
/* B gathers in one launch (one workgroup per problem; B = 1: sage_match_points itself) and one wait; K, W, the camera and the
 * scalars are shared.  M_host [B];
 * mean_noise_depth_host [B] or NULL.  SAGE_E_INVALID as sage_match_points per item, for B < 0 or B > SAGE_REG_MAX_BATCH and
 * for NULL items or M_host with B > 0.  B = 0: SAGE_OK, nothing launched. */
int sage_match_points_batch(SageWorkspace *ws, const SageMatchPointsItem *items, int B, float depth_divisor0, const SageCamera *cam,
                            int K, int W, float noise_multiplier, int noise_from, int32_t *M_host /* [B] */,
                            float *mean_noise_depth_host /* [B] or NULL */);

/* ---- the loop detector's candidates: one query keyframe against B candidates in one call ----
 * LoopDetector::DetectLoop (core/system/loop_detector.cpp:143-163) and DetectLocalLoop (:282-319) run
 * CameraTracker::MatchGeoCheck on the query keyframe against up to loop_max_candidates = 20 (loop_local_active_window = 9)
 * candidates one after the other: "pre check ... for computation speedup".
 *
 * sage_cycle_match_batch: row b of raw_matched_loc1d, cyc_matched_loc1d, inlier_flags (device, [B][K]) and n_inliers_host
 * (HOST, [B]) is what sage_cycle_match(ws, desc_query_dev, desc_cand_dev[b], kp_loc1d_dev[b], ...) writes, bit for bit, for every
 * value of pixel_slices.  desc_cand_dev and kp_loc1d_dev are HOST arrays of B device pointers ([C,H,W] maps; [K] pixels of
 * the query map: per candidate the keypoint set is its own -- camera_tracker.cpp:589-608 shuffles the query's valid locations
 * with the candidate's id as seed; that shuffle stays with the caller, sage_shuffle_indices).  The grid runs over (pixel
 * slice, group of 8 queries, candidate); a slice is a contiguous pixel range of the target map and the winner over the
 * slices is the maximum under one total order (larger response, then smaller pixel), so the split never shows in the result.
 * pixel_slices 0: chosen from the device's CU count, as many as it takes to put two workgroups on every CU and none shorter
 * than 512 pixels; >= 1: forced (clamped to H*W and to 8192; the slices' winners take 16 B K slices bytes of the workspace).
 * Three launches whatever B; the counts reach the host through pinned memory and the workspace's ticket: one wait, no copy.
 * SAGE_E_INVALID, before anything touches the device, for: NULL ws; B < 0 or B > SAGE_MATCH_MAX_BATCH; K < 0 (or K > 524 280);
 * C < 1 or C > 1024; H or W < 1 (or H*W >= 2^31); pixel_slices < 0; NULL n_inliers_host with B > 0; with B > 0 and K > 0 a
 * NULL map, output, pointer array or entry of a pointer array.  B = 0 or K = 0: SAGE_OK, the counts zeroed, nothing launched. */
#define SAGE_MATCH_MAX_BATCH 32
#define SAGE_TRACK_MAX_BATCH 32 /* sage_track_lm_batch, sage_track_frame_batch, sage_loop_verify */
int sage_cycle_match_batch(SageWorkspace *ws, const float *desc_query_dev, const float *const *desc_cand_dev,
                           const int64_t *const *kp_loc1d_dev, int B, int K, int C, int H, int W, float cyc_thresh,
                           int pixel_slices, int64_t *raw_matched_loc1d, int64_t *cyc_matched_loc1d, int32_t *inlier_flags,
                           int32_t *n_inliers_host);
/* the number of pixel slices the workspace's last sage_cycle_match_batch ran with (0: none yet, or NULL ws) */
int sage_cycle_match_batch_slices(const SageWorkspace *ws);

/* sage_loop_precheck: the detector's loop body up to the ratio test (MatchGeoCheck -> the first FeatureMatchingGeo overload,
 * camera_tracker.cpp:575-768) for all B candidates.  A host composition, no arithmetic of its own: one
 * sage_cycle_match_batch (pixel_slices 0); then every candidate that can still pass goes through sage_match_points
 * (depth_divisor0 = query_depth_divisor, noise_from 1, scratch outputs of the workspace: one sage_match_points_batch over all
 * of them) and sage_robust_registration (src = pts0, dst = pts1; p->noise_bound is NOT read: it is replaced by
 * (noise_multiplier * mean_noise_depth) / ((cam->fx + cam->fy) / 2) evaluated in fp32 and widened: one
 * sage_robust_registration_batch over the survivors).  Per candidate the fields of the result equal those three calls on the
 * same inputs.
 * The prune: a candidate with (float)n_cycle / (float)K < min_desc_inlier_ratio gets registered = 0, both ratios 0 and no
 * further launch.  That is exact: the reference's desc_match_inlier_ratio is |translation inliers| / K and the translation
 * inliers are among the cycle-consistent matches, so the detector's `continue` (loop_detector.cpp:159, :314) is taken either
 * way; pass max(cfg.min_desc_inlier_ratio, base_desc_ratio).  n_cycle = 0 is the reference's early return (:642-652) and
 * skips the solve whatever the threshold; so do n_matched < 2 and a bound that is not positive and finite (NaN depths).
 * inlier_kp_dev [B][K]: row b holds, in its first reg.n_inliers entries, kept[inliers[i]] ascending -- positions among the K
 * keypoints, what TrackFrame(..., match_geom_pre_checked = true) gathers homo and depths with, next to row b of
 * raw_matched_loc1d.  raw_matched_loc1d, inlier_flags: device [B][K], as sage_cycle_match_batch writes them.
 * SAGE_E_INVALID (nothing is launched) as for sage_cycle_match_batch, and for NULL cands, cam, p or results, a NULL member of a
 * candidate, fx / fy not positive and finite, K > SAGE_REG_MAX_POINTS; the registration's parameter checks answer as in
 * sage_robust_registration (noise_bound apart).  B = 0 or K = 0: SAGE_OK, the results zeroed.  Waits: four whatever B -- one
 * for the cycle-match batch, one for the gathers, one for the votes, one at the end when any inlier was written.  The
 * workspace's scratch holds the B candidates' gathered points (48 K bytes each) and the batch of votes (above). */
typedef struct SageLoopCandidate /* device pointers */
{
  const float *desc_dev;           /* kf->feat_desc [C,H,W] */
  const float *dpt_map_dev;        /* kf->dpt_map [H*W] */
  const int64_t *kp_loc1d_dev;     /* [K] query pixels of this candidate's keypoints */
  const float *kp_dpts0_dev;       /* [K] the query's depths at them */
  const float *kp_homo0_dev;       /* [K][3] the query's homogeneous coordinates at them */
} SageLoopCandidate;
typedef struct SageLoopPrecheckResult /* host */
{
  int32_t n_cycle;                 /* cycle-consistent matches */
  int32_t n_matched;               /* M of sage_match_points (0: pruned) */
  int32_t registered;              /* 1 when the solve ran */
  float relative_desc_match_inlier_ratio, desc_match_inlier_ratio; /* camera_tracker.cpp:740-741 */
  float mean_noise_depth;
  SageRegistrationResult reg;
} SageLoopPrecheckResult;
int sage_loop_precheck(SageWorkspace *ws, const float *desc_query_dev, float query_depth_divisor, const SageLoopCandidate *cands,
                       int B, int K, int C, int H, int W, const SageCamera *cam, float cyc_thresh, float noise_multiplier,
                       float min_desc_inlier_ratio, const SageRegistrationParams *p, SageLoopPrecheckResult *results,
                       int64_t *raw_matched_loc1d, int32_t *inlier_flags, int32_t *inlier_kp_dev);

/* sage_loop_verify: the detector's loop body after the ratio test -- TrackFrame(*curr_kf, true, use_match_geom, ...,
 * match_geom_pre_checked = true) of loop_detector.cpp:165 / :321 (camera_tracker.cpp:1312-1672) for every survivor of
 * sage_loop_precheck at once.  The accept / sort / redundancy filtering of loop_detector.cpp:173-229 stays with the caller.
 * Survivors: pre[b].registered == 1 and pre[b].reg.n_inliers > 3 (camera_tracker.cpp:1407).  cands, pre, raw_matched_loc1d
 * and inlier_kp_dev are sage_loop_precheck's arrays as they are.
 * A host composition around ONE kernel of its own:
 *   1. one gather launch over (survivor, inlier) builds every survivor's keypoint term (camera_tracker.cpp:1415-1424,
 *      :654-678) into kp_gathered_dev [B][8 K], row b = homo0 [K][3] | unscaled dpts0 [K] | homo1 [K][3] | dpts1 [K], the first
 *      reg.n_inliers entries of each written.  With i = inlier_kp_dev[b][j], loc = raw_matched_loc1d[b][i]:
 *        homo0 = cands[b].kp_homo0_dev[i];  unscaled dpts0 = cands[b].kp_dpts0_dev[i] / query_depth_divisor (a true division)
 *        homo1 = ((fmod((float)loc, W) - cx) / fx, (floor((float)loc / W) - cy) / fy, 1);  dpts1 = cands[b].dpt_map_dev[loc]
 *      -- sage_match_points' expressions, from the same device function (a location outside the map reads a NaN depth);
 *      cam = query->pyr.cam[0], W = cam.w;
 *   2. start values from the registration (:750-761): pose12 = (float)reg.R, (float)reg.t; scale = (float)reg.scale;
 *   3. kp_weight = pre[b].desc_match_inlier_ratio * match_geom_factor_weight (:414, :742), kp_loss_param from the candidate
 *      (match_geom_loss_param_factor * avg_squared_dpt_bias of that keyframe, :409); cfg->no_overlap_error is not read: the
 *      check is off with the match-geometry term (:1515);
 *   4. one sage_track_frame_batch (dof 7, photometric + match geometry) over the survivors: the query's photometric side is
 *      shared, feat1 / grad1 / mask1 are the candidate's;
 *   5. one sage_track_overlap_batch over the survivors the tracker returned SAGE_OK for, in survivor order, with
 *      depth_scale = scale_b / query_depth_divisor (:1644): three launches whatever their number.
 * Per candidate the result equals sage_track_frame + sage_track_overlap on the gathered inputs, byte for byte.  A candidate
 * that is no survivor gets tracked = 0 (the rest of its result zeroed) and no launch beyond the gather, which skips it.
 * SAGE_E_INVALID (nothing is launched) for: NULL ws, cfg, query, results; B < 0 or B > SAGE_TRACK_MAX_BATCH; K < 0 or
 * K > SAGE_REG_MAX_POINTS; with B > 0: NULL cands, vcands, pre, raw_matched_loc1d, inlier_kp_dev or kp_gathered_dev, a
 * query with N < 1, M < 1, FS not 16 / 32, pyr.levels outside 1..SAGE_MAX_LEVELS, a NULL array, fx / fy of pyr.cam[0] not
 * positive and finite; a divisor that is not positive and finite; for a survivor: a NULL member of cands[b] / vcands[b],
 * reg.n_inliers > K.  B = 0 or no survivor: SAGE_OK, the results zeroed.
 * Waits: the rounds of sage_track_frame_batch (one each), then one (the overlap batch). */
typedef struct SageLoopVerifyQuery /* device pointers: the query keyframe's side of every survivor's problem */
{
  int32_t N, FS;                    /* sampled pixels, feature channels */
  const float *homo_dev;            /* [N,3] */
  const float *unscaled_dpts0_dev;  /* [N] dpt_map_0 / dpt_scale_0 at the samples */
  const float *feat0s_dev;          /* [L,N,FS] pre-sampled source features */
  const float *weights_dev;         /* [L] */
  SagePyramid pyr;
  float eps;
  int32_t M;                        /* valid pixels of the query (sage_track_overlap) */
  const float *valid_homo_dev;      /* [M,3] */
  const float *valid_dpts0_dev;     /* [M] dpt_map_0 at them (scaled: depth_scale divides by query_depth_divisor) */
  const float *mask_dev;            /* [h,w] the mask of sage_track_overlap */
} SageLoopVerifyQuery;
typedef struct SageLoopVerifyCandidate /* device pointers, next to cands[b] */
{
  const float *feat1_dev, *grad1_dev, *mask1_dev; /* [FS,P], [2,FS,P], [h,w] of the candidate keyframe */
  float kp_loss_param;
} SageLoopVerifyCandidate;
typedef struct SageLoopVerifyResult /* host */
{
  int32_t tracked;                  /* 0: not a survivor, nothing else is meaningful */
  int32_t status;                   /* SAGE_OK (the match-geometry term switches the no-overlap exit off) */
  float pose12[12], scale, error;
  int32_t iters;
  float area_ratio, inlier_ratio, average_motion; /* sage_track_overlap's three */
  float area_inlier_ratio;          /* area_ratio * inlier_ratio (fp32) */
} SageLoopVerifyResult;
int sage_loop_verify(SageWorkspace *ws, const SageLmConfig *cfg, const SageLoopVerifyQuery *query, float query_depth_divisor,
                     const SageLoopCandidate *cands, const SageLoopVerifyCandidate *vcands, const SageLoopPrecheckResult *pre,
                     int B, int K, const int64_t *raw_matched_loc1d, const int32_t *inlier_kp_dev,
                     float match_geom_factor_weight, float *kp_gathered_dev, SageLoopVerifyResult *results);

/* sage_loop_accept: the rest of the detector's loop body and what follows it (loop_detector.cpp:173-229) -- the accept
 * test, the pose hand-over, df::CorrectDepthScale of every accepted candidate, the sort and the redundancy filter: from
 * sage_loop_verify's results to the filtered LoopInfo list DetectLoop returns.  cands, pre and ver are the arrays of
 * sage_loop_precheck and sage_loop_verify as they are.  A host composition; its only device work is ONE
 * sage_depth_scale_ratio_batch (drop_nan = 1, no per-point outputs) over the accepted candidates.  All arithmetic is fp32.
 *   Accepted (:165-183): ver[b].tracked, ver[b].status == SAGE_OK, ver[b].area_ratio >= min_area_ratio and
 *     ver[b].inlier_ratio >= min_inlier_ratio (:173), metric = ver[b].area_inlier_ratio >= base_metric and
 *     desc = pre[b].desc_match_inlier_ratio >= base_desc_ratio (:183).  A NaN fails every comparison.
 *   Pose (camera_tracker.cpp:1651-1656, loop_detector.cpp:189-193): with R = pose12[0..8] (row-major), t = pose12[9..11] of
 *     ver[b]: R_cur_ref = R^T (row-major); t_cur_ref[i] = ((-R[0][i]) * t[0] + (-R[1][i]) * t[1]) + (-R[2][i]) * t[2] without
 *     contraction, then (t_cur_ref[i] * dpt_scale) / tracker_ref_scale, left to right.  Stated deviation: the reference
 *     passes the rotation through a Sophus::SO3f quaternion and back; the library does not.
 *   Scale (:194-196): query_scale = the ratio of row b of one batch over the accepted candidates in candidate order, with
 *     R10 = R_cur_ref, t10 = the rescaled translation, dpt0_dev = cands[b].dpt_map_dev read at scands[b].valid_loc1d_dev,
 *     homo0_dev = scands[b].valid_homo_dev, M = scands[b].M, the query's bias, mask and camera, eps = dpt_eps;
 *     scale = that row's statistics; ref_scale = scands[b].dpt_scale; desc_inlier_ratio = desc; metric = metric;
 *     id_ref = scands[b].id.
 *   Sort (:207): the accepted candidates by desc_inlier_ratio, descending.  The reference's std::sort leaves the order of
 *     equal ratios unspecified; here ties keep candidate order.
 *   Redundancy filter (:210-228): the first of that order is kept; a later one is kept unless |id - id_kept| <
 *     redundant_range for some candidate kept before it.  kept_order [B]: the kept candidates' indices in that order (the
 *     rest -1); *n_kept: their number.
 * infos [B] is in candidate order: a candidate that is not accepted has accepted = kept = 0 and the rest zeroed.
 * No accepted candidate: SAGE_OK, *n_kept = 0, nothing is launched.
 * SAGE_E_INVALID (nothing is launched) for: NULL ws, cfg, query, infos, kept_order or n_kept; B < 0 or
 * B > SAGE_TRACK_MAX_BATCH; with B > 0 NULL cands, scands, pre or ver; for an accepted candidate: a NULL dpt_map_dev,
 * valid_loc1d_dev or valid_homo_dev, M <= 0, a dpt_scale or tracker_ref_scale that is not positive and finite; with an
 * accepted candidate: a NULL bias_dev or video_mask_dev, a camera sage_depth_scale_ratio refuses.  One wait. */
typedef struct SageLoopAcceptConfig
{
  float min_area_ratio, min_inlier_ratio, base_metric, base_desc_ratio;
  int64_t redundant_range;         /* cfg_.global_redundant_range */
  float dpt_eps;
} SageLoopAcceptConfig;
typedef struct SageLoopScaleQuery /* the keyframe to scale: device pointers [h,w] and its level-0 camera */
{
  const float *bias_dev, *video_mask_dev;
  SageCamera cam;
} SageLoopScaleQuery;
typedef struct SageLoopScaleCandidate /* next to cands[b]: the depth map is cands[b].dpt_map_dev */
{
  int64_t id;                      /* kf->id */
  const int64_t *valid_loc1d_dev;  /* [M] kf->valid_locations_1d */
  const float *valid_homo_dev;     /* [M,3] kf->valid_locations_homo */
  int32_t M;
  float dpt_scale;                 /* kf->dpt_scale */
  float tracker_ref_scale;         /* GetRefScale() after this candidate's TrackFrame */
} SageLoopScaleCandidate;
typedef struct SageLoopInfo /* host */
{
  int32_t accepted, kept;
  int64_t id_ref;
  float R_cur_ref[9], t_cur_ref[3];
  float query_scale, ref_scale, desc_inlier_ratio, metric;
  SageDepthScaleStats scale;
} SageLoopInfo;
int sage_loop_accept(SageWorkspace *ws, const SageLoopAcceptConfig *cfg, const SageLoopScaleQuery *query,
                     const SageLoopCandidate *cands, const SageLoopScaleCandidate *scands, const SageLoopPrecheckResult *pre,
                     const SageLoopVerifyResult *ver, int B, SageLoopInfo *infos /* [B] in candidate order */,
                     int32_t *kept_order /* [B] */, int32_t *n_kept);

/* =====================================================================
 * Batched window engine (no reference counterpart; parity = sum of per-edge results)
 * ===================================================================== */
typedef struct SageWindow SageWindow;

typedef struct SageKeyframeView /* device pointers, reference layouts (core/mapping/frame.h:17-125) */
{
  const float *feat_pyr;  /* [FS,P]   */
  const float *grad_pyr;  /* [2,FS,P] */
  const float *bias;      /* [H*W]    */
  const float *basis;     /* [H*W,CS] */
  const int64_t *loc1d;   /* [N]      */
  const float *homo;      /* [N,3]    */
  int32_t N;
} SageKeyframeView;

typedef struct SageWindowConfig
{
  SagePyramid pyr;
  int32_t FS, CS;
  const float *mask_dev;        /* shared video mask [H,W] */
  float photo_weights[SAGE_MAX_LEVELS];
  float geo_weight, geo_loss_param, eps;
  float code_prior_weight;      /* code_factor_weight (slam_run.flags:104) */
  float scale_prior_weight;     /* init_scale_prior_weight on keyframe 0 */
  float pose_prior_weight;      /* init_pose_prior_weight on keyframe 0 */
  int32_t use_photo, use_geo;
} SageWindowConfig;

int sage_window_create(const SageWindowConfig *cfg, void *hip_stream, SageWindow **out);
void sage_window_destroy(SageWindow *w);
/* variables: pose12 (R,t), code[CS], scale -- HOST pointers, copied. Returns keyframe id >= 0. */
int sage_window_add_keyframe(SageWindow *w, const SageKeyframeView *view, const float *pose12,
                             const float *code, float scale);
/* a link contributes both directed edges of every enabled factor type (mapper.cpp:346-374). */
int sage_window_add_link(SageWindow *w, int kf_a, int kf_b);
/* the Cauchy parameter of ONE link's two geometric edges (before finalize; 0 = the window's geo_loss_param): the mapper
 * derives it per link from the newer keyframe, geo_loss_param_factor * kf->avg_squared_dpt_bias (mapper.cpp:367-373) */
int sage_window_set_link_geo_loss(SageWindow *w, int link, float loss_param);
/* a link that carries keypoint terms only (mapper.cpp:393-446 EnqueueLink with a subset of the factor types; the links of
 * DeepFactors::LoopClosurePoseScaleMGEstimate, core/deepfactors.cpp:388-575): it contributes no photometric or geometric
 * edge, whatever use_photo / use_geo say, but it is part of the solver's structure and owns a link block of the packed
 * buffer.  Returns a link id in the numbering of sage_window_add_link, so `edge = 2 * link + direction` addresses its two
 * directions in sage_window_add_keypoint_term; ownership of those directions on a sharded window follows the same rule as
 * every other link's.  sage_window_get_edge / sage_window_factor on such a link answer SAGE_E_INVALID.  A window whose links
 * are all of this kind launches no dense kernel and still assembles, reduces, solves and iterates.  Before finalize
 * (SAGE_E_STATE afterwards). */
int sage_window_add_keypoint_link(SageWindow *w, int kf_a, int kf_b);
/* held variables: the parts of keyframe `kf` named by the mask `what` keep their values through every solve -- their rows
 * and columns of the damped system are replaced by the identity (no off-diagonal element, right-hand side 0, no prior), so
 * their delta is exactly zero, the free variables see the system with the held ones eliminated at their current values,
 * and the candidate copies them bit for bit.  0 clears.  The packed buffer, the all-reduce payload and the per-edge results
 * are untouched: every factor is still evaluated, and the prior ERROR terms of held variables stay in the total (constants).
 * sage_window_set_keyframe on a held keyframe still sets it.  Before finalize (SAGE_E_STATE afterwards); SAGE_E_INVALID for
 * a bad keyframe or mask.  A window that uses the domain-decomposed solve and holds anything answers SAGE_E_UNSUPPORTED at
 * finalize.
 * Solver rows: a group (pose, code or scale) that EVERY keyframe of the window holds is left out of the damped system
 * altogether -- the solver then works on blocks of the remaining groups' rows, in block order pose / code / scale
 * (sage_window_solver_block_size: 7 when all codes are held, 6 with codes and scales, 1 + CS with all poses), instead of
 * carrying identity rows: less to stream to the host, less to factorise.  A group that a single keyframe leaves free is
 * kept whole, its held rows as identity rows inside the smaller block; a window that holds nothing, or everything, solves at
 * B.  The step is the same either way; sage_window_block_size, the packed buffer and sage_window_get_delta keep the layout
 * of B rows per keyframe, dropped rows with delta 0. */
enum { SAGE_HOLD_POSE = 1, SAGE_HOLD_CODE = 2, SAGE_HOLD_SCALE = 4 };
int sage_window_hold(SageWindow *w, int kf, int what);
/* edge sharding for multi-GPU: this process evaluates the contiguous range [rank*2n/world, (rank+1)*2n/world) of the 2n
 * DIRECTED edges (edge 2l = link l a -> b, 2l + 1 = b -> a, links in the order they were added; both factor types of a
 * direction together) -- r05: the two directions of a link may sit on two ranks (42 links on 8 ranks are 5 or 6 each, 84
 * directed edges 10 or 11).  Windows that use the domain-decomposed solve (SAGE_SHARD_SCHUR, default from 256 keyframes)
 * shard by whole links, [rank*n/world, (rank+1)*n/world), as sage_shard_plan_create assumes.  Default (0,1). */
int sage_window_set_shard(SageWindow *w, int rank, int world);
/* must be called once after the last add_keyframe/add_link and before linearize/error. */
int sage_window_finalize(SageWindow *w);

int sage_window_num_keyframes(const SageWindow *w);
int sage_window_num_links(const SageWindow *w);
int sage_window_block_size(const SageWindow *w);       /* B = 7 + CS: [pose6, code CS, scale] */
int sage_window_solver_block_size(const SageWindow *w); /* Bs <= B: rows per keyframe in the solver (sage_window_hold); 0
                                                          * before finalize or for NULL */
/* packed normal-equation buffer (device, DOUBLE), the all-reduce payload:
 *   [ diag blocks K*B*B | link blocks nlinks*B*B (row = older kf, col = newer kf) | g K*B | err_photo err_geo n_photo n_geo ]
 * (windows with keypoint terms: err_photo also carries the reprojection terms' errors, err_geo the match-geometry, loop-MG and graph terms';
 * the two inlier counts stay dense-only -- see sage_window_add_keypoint_term)
 * fp32 per-edge results are summed in double, like the reference widens AtA/Atb to double before gtsam adds
 * the factors (core/gtsam/photometric_factor.cpp:305-306); keeping the payload in double keeps the sum exact
 * across ranks too. */
size_t sage_window_packed_count(const SageWindow *w);
double *sage_window_packed_dev(SageWindow *w);
/* number of residuals one linearize evaluates on this shard (E_photo*L*N*FS + E_geo*N, + 2N / 3N per reprojection /
 * match-geometry / loop-MG term, + 7 / 6 / 1 per graph term) and its algorithmic bytes (dense factors) */
double sage_window_residuals_per_linearize(const SageWindow *w);
double sage_window_bytes_per_linearize(const SageWindow *w);

/* linearize every local edge at the current estimate and assemble the packed buffer (async on the stream). */
int sage_window_linearize(SageWindow *w);
/* total error of every local edge at the CANDIDATE (or current, which = 0/1) variables -> 4-double device
 * buffer [err_photo err_geo n_photo n_geo]; async. */
int sage_window_error(SageWindow *w, int which);
/* (no reference counterpart) run-length tuning of the photometric kernels on the window's own data: times the photometric
 * linearize + error pass with workgroup runs of 4 ... 16 sub-tiles at the current estimate (three timed evaluations per candidate) and keeps
 * the fastest when it beats the static rule's choice by >= 4 %.  Opt-in -- call it once after sage_window_finalize (or set
 * SAGE_AUTOTUNE=1, then finalize calls it); SAGE_PHOTO_TPB pins the run length and turns this into a no-op, as does a sharded
 * window.  Results are bit-reproducible for a given run length, not across run lengths (different fp32 summation order).
 * Side effects: the system the timed evaluations left in the packed buffer was assembled under whichever plan was measured
 * last and is dropped -- a linearize must follow (sage_window_lm_step does its own; sage_window_solve answers SAGE_E_STATE
 * until then); the kernel-time records of sage_window_set_profiling are consumed (the profiling switch itself is restored).
 * Outputs (any may be NULL): the run length now in use, the rule's, and the two timings in ms (0 when nothing was measured). */
int sage_window_tune_runs(SageWindow *w, int *tpb_out, int *tpb_rule_out, float *ms_rule_out, float *ms_best_out);
/* re-apply a run length found by sage_window_tune_runs on an earlier window of the same geometry (1 <= tpb <= 64).  A system
 * linearized before the call belongs to the previous plan and is dropped: a linearize must follow, as above. */
int sage_window_set_runs(SageWindow *w, int tpb);
double *sage_window_error_dev(SageWindow *w);
/* after (optional) all-reduce of the packed buffer: add priors, D2H, damped solve in double on the host,
 * write the candidate variables (retracted) and upload them.  Returns the predicted step norm. */
int sage_window_solve(SageWindow *w, double damp, double *step_norm);
/* total error (photo + geo + priors) from the (all-reduced) buffers; synchronises. */
int sage_window_total_error(SageWindow *w, int from_linearize, double *err);
int sage_window_accept(SageWindow *w);   /* candidate -> current */
int sage_window_reset(SageWindow *w);    /* restore the variables every keyframe was added with */
/* read back current variables (HOST outputs; any may be NULL) */
int sage_window_get_keyframe(const SageWindow *w, int kf, float *pose12, float *code, float *scale);
int sage_window_set_keyframe(SageWindow *w, int kf, const float *pose12, const float *code, float scale);
/* host copy of the last solve's delta (K*B doubles), for parity tests */
int sage_window_get_delta(const SageWindow *w, double *delta);
/* host copy of per-edge results of the last linearize, reference layouts (for parity tests):
 * type 0 = photometric (D=13+CS), 1 = geometric (D=14+2CS); edge index e in [0, 2*nlinks): link e/2,
 * direction e%2 (0: a->b, 1: b->a).  After sage_window_linearize / sage_window_prepass: one factor type per result,
 * exactly the reference's per-edge AtA / Atb.  After sage_window_lm_step (windows with both factor types): the iteration's
 * MERGED linearize -- the geometric edge's blocks that involve code0 through kappa*b0 (code0-code0, pose-code0, scale0-code0,
 * code0 gradient) ride in the PHOTOMETRIC edge's result of the same pair and read zero in the geometric one; the sum of
 * the two -- what the assembly forms -- is the same normal equations. */
int sage_window_get_edge(const SageWindow *w, int type, int e, float *AtA, float *Atb, float *err, float *n_in);

/* Matched-keypoint terms on the directed edges of a window: the mapper's third factor type (core/mapping/mapper.cpp:346-374
 * adds photometric, reprojection and geometric factors per link and direction; demo/main.cpp:254-278: weight 5, loss
 * 0.1 W^2, up to 512 keypoints).  Same arithmetic as the per-edge operators below (sage_reprojection_jac_error_calculate,
 * sage_match_geometry_jac_error_calculate), but every term of the window is evaluated in ONE launch per linearize / error
 * pass and summed into the same packed system and error totals as the dense factors, so sage_window_solve, sage_window_lm_step
 * and the sharded sequences see them without knowing.
 *   kind SAGE_KP_REPROJECTION    fair loss, D = 13+CS [pose0 pose1 code0 scale0] (the photometric edge layout), 2N residuals
 *   kind SAGE_KP_MATCH_GEOMETRY  loss SAGE_LOSS_*, D = 14+2CS [pose0 pose1 code0 code1 scale0 scale1] (the geometric edge
 *                                layout), 3N residuals
 *   kind SAGE_KP_LOOP_MG         fair loss, D = 14 [pose0 pose1 scale0 scale1], 3N residuals: match geometry with the depths
 *                                fixed at graph-build time (LoopMGFactor, core/deepfactors.cpp:388-575; the arithmetic of
 *                                sage_loop_mg_jac_error_calculate).  The two unscaled depth arrays are the caller's; poses
 *                                and scales are the window's.  loc1d_0, matched_loc1d_1 and loss are ignored (may be NULL /
 *                                0); loss_param > 0.  No code row or column of the system receives anything from it.
 * `edge` = 2 * link + direction as sage_window_get_edge numbers them; keyframe "0" is the direction's source.  Camera =
 * cfg.pyr.cam[0], eps = cfg.eps; bias / basis / code / scale / pose are the window's keyframes' at the variable set being
 * evaluated.  Add after the edge's link and before sage_window_finalize (SAGE_E_STATE afterwards); any number of terms per
 * edge; SAGE_E_INVALID for a bad edge / kind / loss, N < 1 (the reference adds no factor without matches,
 * core/mapping/df_work.cpp:416), a missing array or a location outside the image.  The arrays are DEVICE memory and are
 * copied by the call (unlike the keyframe views): the caller may free them afterwards.  Returns the term id >= 0: ids count
 * the add calls of the whole window.  On a sharded window a term belongs to the rank that owns its directed edge (settled at
 * finalize: add and sage_window_set_shard may come in either order); reading a term of another rank answers SAGE_E_INVALID.
 * get_keypoint_term: host copy of the term's last linearize in the reference's per-edge layout (AtA [D,D], Atb [D], error;
 * n_in = inliers for reprojection, N for match geometry and loop-MG); SAGE_E_STATE before the first linearize.
 * Totals: the terms' errors ride in the two error slots of the 4-double tails (packed buffer, error buffer) -- reprojection in
 * the photometric slot, match geometry and loop-MG in the geometric one: slot 0 + slot 1 = sum of dense + sum of keypoint
 * errors.  The inlier slots stay dense-only.  The gtsam factor cache serves the terms as well: sage_window_prepass caches
 * them and sage_window_keypoint_factor hands out their HessianFactor blocks (below, next to sage_window_factor). */
enum { SAGE_KP_REPROJECTION = 0, SAGE_KP_MATCH_GEOMETRY = 1, SAGE_KP_LOOP_MG = 2 };
typedef struct SageKeypointTerm
{
  int32_t kind;                   /* SAGE_KP_*                                                          */
  int32_t edge;                   /* directed edge 2*link + direction, numbered as sage_window_get_edge */
  int32_t N;                      /* matched keypoints, >= 1                                            */
  const int32_t *loc1d_0;         /* [N]   device: flat pixel of the keypoint in the edge's keyframe "0" */
  const float *homo0;             /* [N,3] device                                                       */
  const float *matched_2d;        /* reprojection:   [N,2] device, pixels in keyframe "1"               */
  const int32_t *matched_loc1d_1; /* match geometry: [N]   device                                       */
  const float *matched_homo1;     /* match geometry: [N,3] device                                       */
  float loss_param, weight;
  int32_t loss;                   /* match geometry: SAGE_LOSS_*; ignored for reprojection              */
  const float *unscaled_dpts0, *matched_unscaled_dpts1; /* loop-MG: [N] device each, depths before their keyframe's scale */
} SageKeypointTerm;
int sage_window_add_keypoint_term(SageWindow *w, const SageKeypointTerm *t);
int sage_window_num_keypoint_terms(const SageWindow *w);
int sage_window_get_keypoint_term(const SageWindow *w, int term, float *AtA, float *Atb, float *err, float *n_in);

/* Pose-graph terms of a window: the factors of the graph the reference solves after every accepted global loop,
 * DeepFactors::LoopClosurePoseScaleEstimate (core/deepfactors.cpp:58-386; called at :1134 and :1208).  That graph holds no
 * keypoint: it is RelPoseScaleFactors on both directions of every link, a pose prior and a ScaleFactor on the first keyframe
 * and two ScaleFactors on the newest loop's keyframes.  With R10 = R1^T R0, t10 = R1^T (t0 - t1) of the window's poses and
 * (Rt, tt, ts0, ts1) the term's target, the residuals r = target - current are
 *   kind SAGE_GRAPH_REL_POSE_SCALE  tt / ts0 - t10 / s0 (3), sqrt(rot_weight) (log Rt - log R10) (3),
 *                                   sqrt(scale_weight) (log(ts1 / ts0) - log(s1 / s0)) (1)   (rel_pose_scale_factor.cpp:207-344)
 *   kind SAGE_GRAPH_REL_POSE        tt - t10 (3), sqrt(rot_weight) (log Rt - log R10) (3)     (rel_pose_factor.cpp:150-262)
 *   kind SAGE_GRAPH_SCALE_PRIOR     log(ts0) - log(s) of keyframe `kf` (1)                    (scale_factor.cpp:102-129)
 * and error = weight |r|^2, AtA = weight J^T J, Atb = weight J^T r with J = d current / d [delta0 delta1 s0 s1] under the
 * window's left retraction.  The error is the reference's as written; J is its exact derivative, which differs from the
 * reference's matrix in two places: rel_pose_scale_factor.cpp:288 / rel_pose_factor.cpp:229 form d pose10 / d pose1^-1 as
 * kron(pose0, I3) where the derivative is kron(pose0^T, I3) (its pose1 columns are off by 0.5 to 2 on unit-size inputs; with
 * the transpose the pose1 block is exactly minus the pose0 block), and rel_pose_scale_factor.cpp:320 uses the TARGET's
 * translation in the scale0 column (-tt / s0^2) where the derivative is -t10 / s0^2.  There is no "as written" mode.  log R
 * and its derivative are accurate from the identity (bit-exact zero) to a relative rotation of 2.5 rad; the neighbourhood of
 * pi is outside the reference's formula and outside this one.  No NearestPsd on the window path, as for every other term.
 * `edge` = 2 * link + direction as sage_window_get_edge numbers them; keyframe "0" is the direction's source.  Add after the
 * edge's link (a dense or a keypoint link) and before sage_window_finalize (SAGE_E_STATE afterwards); any number of terms per
 * edge; SAGE_E_INVALID for a bad kind / edge / keyframe, a weight or a target scale of the kind that is not positive, a negative
 * rot_weight / scale_weight, or a target that is not finite.  Host data only, copied by the call.  Returns the
 * term id >= 0 (ids count the graph terms of the window, apart from the keypoint terms').
 * The terms are evaluated in one launch per linearize / error pass and summed into the same packed system and totals as
 * everything else -- only pose and scale rows receive anything; their errors ride in the geometric slot behind the loop-MG
 * terms'; sage_window_residuals_per_linearize counts 7 / 6 / 1 per term.  sage_window_solve, the LM entry points, holds, solver
 * rows and the reduced (sharded) sequences see them without knowing.  On a sharded window a binary term belongs to the rank
 * that owns its directed edge and a scale prior to rank 0; a window of the domain-decomposed solve with a graph term answers
 * SAGE_E_UNSUPPORTED at finalize.
 * get_graph_term: host copy of the term's last linearize in the D = 14 layout [pose0 pose1 scale0 scale1] for every kind
 * (AtA [14,14], Atb [14], error; columns a kind does not have read zero -- a scale prior sits at [12]); SAGE_E_STATE before
 * the first linearize, SAGE_E_INVALID for a term of another rank.
 * LoopClosurePoseScaleEstimate as a window: keypoint links for the graph's links, every code held, keyframe 0's pose held (the
 * sigma = 1e-4 prior), scale_prior_weight = 0 and a weight-100 SAGE_GRAPH_SCALE_PRIOR on keyframe 0 at its scale, two
 * REL_POSE_SCALE terms per link (the second with the inverse target and the scales swapped), SCALE_PRIORs on the newest loop's
 * two keyframes. */
enum { SAGE_GRAPH_REL_POSE_SCALE = 0, SAGE_GRAPH_REL_POSE = 1, SAGE_GRAPH_SCALE_PRIOR = 2 };
typedef struct SageGraphTerm /* host data only, copied by the call */
{
  int32_t kind;
  int32_t edge;                       /* binary kinds: 2*link + direction; keyframe "0" = the direction's source */
  int32_t kf;                         /* SCALE_PRIOR: the keyframe */
  float target_pose10[12];            /* target of pose1^-1 * pose0, R row-major then t */
  float target_scale0, target_scale1; /* > 0; SCALE_PRIOR uses target_scale0 */
  float weight, rot_weight, scale_weight;
} SageGraphTerm;
int sage_window_add_graph_term(SageWindow *w, const SageGraphTerm *t); /* term id >= 0 */
int sage_window_num_graph_terms(const SageWindow *w);
int sage_window_get_graph_term(const SageWindow *w, int term, float *AtA, float *Atb, float *err);

/* f2 (core/gtsam/photometric_factor.cpp:72-219, geometric_factor.cpp:41-233, mapper.cpp:544-551): the
 * batched per-Values prepass behind the gtsam factors.  ISAM2 calls linearize(values) / error(values) factor by factor
 * with the same Values; the adapter's factor hands the window's values over and the engine evaluates the WHOLE window
 * once per distinct Values:
 *   sage_window_prepass(win, pose12[K][12], codes[K][CS], scales[K], jacobians, &recomputed)
 *       values bit-identical to the cached ones and the cache holds what is asked for -> nothing is launched
 *       (*recomputed = 0); otherwise they become the window's current variables, ONE sage_window_linearize
 *       (jacobians != 0) or ONE sage_window_error (jacobians == 0) runs, and the per-edge results are copied to the host
 *       cache (*recomputed = 1).  A cached linearisation also answers error() at the same values.
 *   sage_window_factor(win, type, e, psd_mode, G, g, f, dims, nkeys)
 *       the HessianFactor of directed edge e (as sage_window_get_edge numbers them) from the cache: blocks and g as
 *       sage_factor_hessian_blocks cuts them (NearestPsd per psd_mode), *f = the factor's error_ (the constant term the
 *       reference passes to gtsam::HessianFactor).  SAGE_E_STATE when the cache holds no linearisation.
 *   sage_window_factor_error(win, type, e, &err)     PhotometricFactor::error / GeometricFactor::error from the cache.
 * Host pointers throughout; type 0 = photometric, 1 = geometric.  One window is not re-entrant: callers on several
 * host threads serialise prepass + factor reads per window (integration/sage_gtsam_prepass.h holds a mutex). */
int sage_window_prepass(SageWindow *w, const float *pose12, const float *codes, const float *scales, int jacobians,
                        int *recomputed);
int sage_window_factor(const SageWindow *w, int type, int e, int psd_mode, double *G_out, double *g_out, double *f_out,
                       int *dims_out, int *nkeys_out);
int sage_window_factor_error(const SageWindow *w, int type, int e, double *err_out);
/* Optional, after a prepass with jacobians: NearestPsd (psd_mode as above) of EVERY cached factor on n_threads host threads
 * (0 = a quarter of the host's hardware threads, at most 64).  The projection -- an SVD / eigen-decomposition of a (13+CS)^2 and a (14+2CS)^2 matrix per link
 * direction -- is the host cost of the gtsam path (photometric_factor.cpp:142-149); ISAM2 pays it factor by factor, this
 * pays it once per Values in parallel, and sage_window_factor with the same psd_mode then only cuts blocks.  The next
 * prepass that recomputes invalidates it. */
int sage_window_prepare_factors(SageWindow *w, int psd_mode, int n_threads);
/* the two halves of sage_factor_hessian_blocks: projection of one factor's AtA (double D x D out), block cutting */
int sage_factor_psd(int type, int CS, const float *AtA, int psd_mode, double *C_out);
int sage_factor_cut_blocks(int type, int CS, const double *C, const float *Atb, double *G_out, double *g_out,
                           int32_t *dims_out, int32_t *nkeys_out);

/* The same for a window's terms: the reference's MatchGeometryFactor / ReprojectionFactor (mapper.cpp:346-374) and the
 * loop-closure graphs' LoopMGFactor, RelPoseScaleFactor, RelPoseFactor and ScaleFactor project their own AtA in linearize()
 * and cut it into G11..Gnn.  family: SAGE_TERM_KEYPOINT (kind SAGE_KP_*) or SAGE_TERM_GRAPH (kind SAGE_GRAPH_*).  The kind
 * fixes the keys in push order, their dims, and the columns it owns of the layout sage_window_get_keypoint_term /
 * sage_window_get_graph_term return:
 *   keypoint REPROJECTION     p0 p1 c0 s0         6 6 CS 1        all 13+CS   (= type 0)
 *   keypoint MATCH_GEOMETRY   p0 p1 c0 c1 s0 s1   6 6 CS CS 1 1   all 14+2CS  (= type 1)
 *   keypoint LOOP_MG          p0 p1 s0 s1         6 6 1 1         all 14
 *   graph    REL_POSE_SCALE   p0 p1 s0 s1         6 6 1 1         all 14
 *   graph    REL_POSE         p0 p1               6 6             0..11 of 14
 *   graph    SCALE_PRIOR      s                   1               12 of 14
 * sage_term_factor_block_count: the doubles of G_out (SAGE_E_INVALID for a bad family / kind, CS < 1).
 * sage_term_factor_blocks (host only): AtA [D,D], Atb [D] in the group's layout; the kind's own D_own x D_own sub-matrix is
 * widened to double and projected per psd_mode as sage_factor_psd projects (a RelPoseFactor's 12 x 12, not a padded
 * 14 x 14), its upper blocks are cut in push order into G_out, g_out [D_own] = the kind's columns of Atb widened.
 * dims_out [<= 6], nkeys_out: optional.  SAGE_E_INVALID for a bad family / kind / mode, CS < 1 or a NULL array.
 *   sage_window_keypoint_factor(win, term, psd_mode, G, g, f, dims, nkeys), sage_window_graph_factor(..)
 *       the HessianFactor of term `term` (the id its add call returned) from the cache of the last linearising
 *       sage_window_prepass, which on a window with terms also copies every term group's results to the host: blocks and g
 *       as sage_term_factor_blocks cuts them from the cached system, bit for bit; *f = the term's error.  Every output
 *       pointer but G_out and g_out may be NULL.  SAGE_E_STATE when the cache holds no linearisation, SAGE_E_INVALID for a
 *       bad id or mode, a NULL G_out / g_out, or a term of another rank (as sage_window_get_keypoint_term answers).
 *   sage_window_keypoint_factor_error(win, term, &err), sage_window_graph_factor_error(..)
 *       the term's error from the cache (of a linearising prepass or of an error-only one); SAGE_E_STATE without either.
 * Both eager projections cover the terms: sage_window_prepare_factors queues every term's own D_own x D_own matrix with the
 * dense factors (longest jobs first), sage_window_prepare_factors_device adds one launch per term group that has entries, at
 * the group's D.  There the D = 14 group is projected as it lies -- a REL_POSE or SCALE_PRIOR term inside its zero-padded
 * 14 x 14, whose zero rows the sweeps skip and the acceptance test passes -- so such a term's blocks are a projection of
 * the same matrix with another rotation order, within the parity bar of the batched projection at the kind's own D.  After
 * either, a term's factor of the prepared mode is cut from the prepared matrix. */
enum { SAGE_TERM_KEYPOINT = 0, SAGE_TERM_GRAPH = 1 };
int sage_term_factor_block_count(int family, int kind, int CS);
int sage_term_factor_blocks(int family, int kind, int CS, const float *AtA, const float *Atb, int psd_mode, double *G_out,
                            double *g_out, int32_t *dims_out, int32_t *nkeys_out);
int sage_window_keypoint_factor(const SageWindow *w, int term, int psd_mode, double *G_out, double *g_out, double *f_out,
                                int32_t *dims_out, int32_t *nkeys_out);
int sage_window_keypoint_factor_error(const SageWindow *w, int term, double *err_out);
int sage_window_graph_factor(const SageWindow *w, int term, int psd_mode, double *G_out, double *g_out, double *f_out,
                             int32_t *dims_out, int32_t *nkeys_out);
int sage_window_graph_factor_error(const SageWindow *w, int term, double *err_out);

/* The projection of psd_mode 1 (sage_nearest_psd: the Higham projection) for n matrices at once on the device, one
 * workgroup per matrix, everything in LDS and in fp64:
 *   1. B = (M + M^T) / 2 from the fp32 row AtA_dev[i].  A non-finite entry: C_dev[i] = B as it is, status 2, done.
 *   2. B = V diag(w) V^T by parallel cyclic two-sided Jacobi: a sweep is D - 1 rounds (D even) or D rounds (D odd), the
 *      D / 2 disjoint pairs of a round (sage_jacobi_round_pairs) are rotated at once with the rotation of the host's
 *      Jacobi fallback.  Before every sweep off = the off-diagonal and diag = the diagonal sum of squares are measured;
 *      the sweeps end at off <= (2^-52)^2 diag, or after 30 sweeps with status 1.
 *   3. H = V |w| V^T, A3 = (B + H) / 2 on one triangle, mirrored: C is symmetric bit for bit.
 *   4. The acceptance test and bump loop of sage_nearest_psd: an unpivoted LDL^T (every pivot >= 0, a zero pivot zeroes
 *      its column and, stricter than the host's test, fails when that column is not zero already; the device's own
 *      summation order); while it fails, at most 60 times, max(-mn k + 1e-15, one ulp of
 *      the largest |diagonal entry|) is added to the diagonal, k = 1, 2, 4, ..; mn = min_i (w_i + |w_i|) / 2, the
 *      smallest eigenvalue of A3 up to rounding, plus the bumps so far.
 * A matrix's result does not depend on the rest of the batch or on its place in it, byte for byte.  No atomics.
 * SagePsdStats: status 0 ok, 1 sweep cap reached (C is the projection with the V and w reached), 2 non-finite input (sweeps,
 * bump_rounds, min_eig, off_norm all 0), 3 the test still failed after the 60th bump (C as bumped; the host loop ends there
 * too, without a word); sweeps, bump_rounds: as counted above; min_eig: the smallest w; off_norm: sqrt(off)
 * as last measured.
 * sage_factor_psd_batch: AtA_dev [n][D][D] float and C_dev [n][D][D] double on the device, stats_host [n] on the host or
 * NULL.  The projection kernel and the workspace's ticket kernel, one wait, whatever n.  SAGE_E_INVALID, before anything
 * touches the device: NULL ws, AtA_dev or C_dev; D < 1 or D > SAGE_PSD_MAX_DIM; n < 0.  n = 0: SAGE_OK, nothing launched.
 * sage_factor_psd_batch_launches: what the workspace's last call launched.
 * sage_factor_psd_batch_plan (host only; every output pointer may be NULL; SAGE_E_INVALID for D or n out of range), with
 * Dc = D rounded up to a multiple of 16, the capacity the kernel is instantiated for:
 *   lds_bytes    = 8 (2 Dc (Dc | 1) + 4 Dc + 64)    the two matrices at the widest row stride, four vectors, the sums' slots
 *   device_bytes = 12 n D D                         the input and the output; the call itself reserves none
 *   pinned_bytes = 32 n                             the records
 *   launches     = 2, or 0 for n = 0
 * Inside a workgroup the row stride is D | 1 doubles and a round's pairs take 16 lanes each: 8 Dc lanes.
 * sage_jacobi_round_pairs (host only): the pairs of `round` as the kernel rotates them, pairs [2 (D / 2)] = p0 q0 p1 q1 ..
 * with p < q; returns their number D / 2 (0 for D = 1), or SAGE_E_INVALID for D out of range, a round outside the sweep or
 * NULL pairs. */
#define SAGE_PSD_MAX_DIM 80
typedef struct SagePsdStats
{
  int32_t status; /* 0 ok, 1 sweep cap reached, 2 non-finite input, 3 bump cap reached */
  int32_t sweeps, bump_rounds;
  double min_eig;  /* of B */
  double off_norm; /* off-diagonal norm at exit */
} SagePsdStats;
int sage_factor_psd_batch(SageWorkspace *ws, int D, int n, const float *AtA_dev, double *C_dev, SagePsdStats *stats_host);
int sage_factor_psd_batch_launches(const SageWorkspace *ws);
int sage_factor_psd_batch_plan(int D, int n, int64_t *lds_bytes, int64_t *device_bytes, int64_t *pinned_bytes,
                               int32_t *launches);
int sage_jacobi_round_pairs(int D, int round, int32_t *pairs);
/* sage_window_prepare_factors with psd_mode 1, on the device: every cached factor of the last recomputing prepass goes
 * through the kernel of sage_factor_psd_batch -- one launch per factor type present, then one wait -- and the projected
 * matrices land in the cache sage_window_factor with psd_mode 1 reads.  The kernel's input is the window's device AtA
 * while that still is the linearisation the cache was pulled from; after another linearize the cached copy is uploaded
 * first.  A factor whose status is not 0 is projected again on the host by sage_factor_psd, so bad inputs come out as
 * sage_window_prepare_factors leaves them.  worst (optional): the record with the highest status, then the most sweeps,
 * then the most bump rounds.  SAGE_E_STATE without a cached linearisation; SAGE_OK at once, nothing launched, when mode 1
 * is prepared already (by either call).  The next recomputing prepass invalidates it, a sage_window_prepare_factors with
 * another mode replaces it.  sage_window_prepare_factors_device_launches: kernels the last call launched -- the dense
 * factor types present plus the term groups that have entries (2 on a dense window without terms, 5 with all three groups).
 * `worst` ranges over dense factors and terms; a term whose record is not clean is projected on the host as
 * sage_term_factor_blocks projects it. */
int sage_window_prepare_factors_device(SageWindow *w, SagePsdStats *worst);
int sage_window_prepare_factors_device_launches(const SageWindow *w);

/* kernel timing with HIP events on the engine's own stream (bench.py's roofline): when enabled every launch of
 * the hot kernels is bracketed by an event pair.  which: 0 photometric linearize, 1 geometric linearize,
 * 2 photometric error, 3 geometric error, 4 keypoint-term linearize, 5 keypoint-term error, 6 graph-term linearize, 7 graph-term
 * error, 8 prior_eval_kernel (both passes), 9 prior_add_kernel.  get_kernel_time synchronises, returns the accumulated milliseconds and
 * launch count since the last reset, and resets them. */
/* on: 0 off, 1 every hot kernel + the phase marks, 2 the photometric linearize only (two event records per iteration
 * instead of eleven: each record is a few microseconds of the stream's time). */
int sage_window_set_profiling(SageWindow *w, int on);
int sage_window_get_kernel_time(SageWindow *w, int which, double *total_ms, int *launches);
/* phases of the LM iterations run through sage_window_lm_step / _lm_run since the last call (profiling on), on the
 * stream's own timeline (HIP events): ms4 = {linearize (depth maps .. assembled system), all-reduce of the system,
 * solve (scatter + host factorisation + retract), error pass}, summed over `iterations`; whatever a step takes beyond
 * their sum is host time with the device idle (accept / reject decision, second all-reduce, launch gaps). */
int sage_window_get_phase_time(SageWindow *w, double *ms4, int *iterations);

/* ---- f3 (first part): sparse reprojection factor with the fair loss ----------------------------------------------
 * Replaces cuda/reprojection_factor_kernels.h:8-46 (reference: reprojection_factor_kernels.cpp):
 *   sage_reprojection_jac_error_calculate   <- reprojection_jac_error_calculate<CS>   (:468-531; kernel :27-213)
 *   sage_reprojection_error_calculate       <- reprojection_error_calculate<CS>       (:417-466; kernel :215-286)
 *   sage_tracker_reproj_jac_error_calculate <- tracker_reproj_jac_error_calculate     (:533-593; kernel :288-366)
 *   sage_tracker_reproj_error_calculate     <- tracker_reproj_error_calculate         (:595-628; kernel :367-415)
 * matched_2d [N,2] are the matched keypoint locations in keyframe 1 (pixels); loc1d is int32 as in the reference;
 * AtA [D,D] / Atb [D] are device arrays, D = 13+CS (mapper: [pose0 pose1 code0 scale0]) or 6 (tracker);
 * error / num_inliers are host scalars (the call synchronises the stream, like the reference's .item<float>()).
 * Without a keypoint in front of the camera: error = 10*weight, AtA = Atb = 0. */
int sage_reprojection_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host,
                                          float *num_inliers_host, const float *R10, const float *t10, const float *R0,
                                          const float *t0, const float *R1, const float *t1, const float *bias0,
                                          const float *basis0, const float *code0, const int32_t *loc1d,
                                          const float *homo, const float *matched_2d, float scale0,
                                          const SageCamera *cam, float eps, float loss_param, float weight, int N, int CS);
int sage_reprojection_error_calculate(SageWorkspace *ws, float *error_host, float *num_inliers_host, const float *R10,
                                      const float *t10, const float *bias0, const float *basis0, const float *code0,
                                      const int32_t *loc1d, const float *homo, const float *matched_2d, float scale0,
                                      const SageCamera *cam, float eps, float loss_param, float weight, int N, int CS);
int sage_tracker_reproj_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host,
                                            float *num_inliers_host, const float *R, const float *t,
                                            const float *sampled_dpts0, const float *homo, const float *matched_2d,
                                            const SageCamera *cam, float eps, float loss_param, float weight, int N);
int sage_tracker_reproj_error_calculate(SageWorkspace *ws, float *error_host, float *num_inliers_host, const float *R,
                                        const float *t, const float *sampled_dpts0, const float *homo,
                                        const float *matched_2d, const SageCamera *cam, float eps, float loss_param,
                                        float weight, int N);

/* ---- f3 (second part): 3-D match-geometry factors ----------------------------------------------------------------
 * Replaces cuda/match_geometry_factor_kernels.h:9-78 (reference: match_geometry_factor_kernels.cpp).  One entry point
 * pair per reference function family; `loss` replaces the reference's robust_loss_type string:
 *   sage_match_geometry_{jac_,}error_calculate  <- match_geometry_{jac_,}error_calculate<CS>   (:1674-1858, :1565-1672)
 *        D = 14+2CS [pose0 pose1 code0 code1 scale0 scale1]; loss SAGE_LOSS_FAIR | _L2 | _HUBER | _UNBIASED
 *   sage_loop_mg_{jac_,}error_calculate          <- loop_mg_{jac_,}error_calculate             (:1510-1563, :1475-1508)
 *        D = 14 [pose0 pose1 scale0 scale1], unscaled depths of the matched points handed over, fair loss
 *   sage_tracker_match_geom_jac_error_calculate  <- tracker_match_geom_jac_error_calculate     (:1388-1431)   D = 6
 *        with_scale != 0: ..._with_scale (:1433-1473), D = 7 (relative pose, scale0)
 *   sage_tracker_match_geom_error_calculate      <- tracker_match_geom_error_calculate         (:1352-1386)
 * All point arrays have N rows (N >= 1: the reference's mean over zero keypoints is NaN; N < 1 is SAGE_E_INVALID);
 * loc1d arrays are int32; error = weight * mean(per-keypoint loss); AtA/Atb device, error host (synchronises). */
enum { SAGE_LOSS_FAIR = 0, SAGE_LOSS_L2 = 1, SAGE_LOSS_HUBER = 2, SAGE_LOSS_UNBIASED = 3 };
int sage_match_geometry_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host,
                                            const float *R10, const float *t10, const float *R0, const float *t0,
                                            const float *R1, const float *t1, const float *bias0, const float *bias1,
                                            const float *basis0, const float *basis1, const float *code0,
                                            const float *code1, const float *homo0, const float *matched_homo1,
                                            const int32_t *loc1d_0, const int32_t *matched_loc1d_1, float scale0,
                                            float scale1, float loss_param, float weight, int loss, int N, int CS);
int sage_match_geometry_error_calculate(SageWorkspace *ws, float *error_host, const float *R10, const float *t10,
                                        const float *bias0, const float *bias1, const float *basis0, const float *basis1,
                                        const float *code0, const float *code1, const float *homo0,
                                        const float *matched_homo1, const int32_t *loc1d_0,
                                        const int32_t *matched_loc1d_1, float scale0, float scale1, float loss_param,
                                        float weight, int loss, int N, int CS);
int sage_loop_mg_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host,
                                     const float *R10, const float *t10, const float *R0, const float *t0,
                                     const float *R1, const float *t1, const float *unscaled_dpts0,
                                     const float *matched_unscaled_dpts1, const float *homo0, const float *matched_homo1,
                                     float scale0, float scale1, float loss_param, float weight, int N);
int sage_loop_mg_error_calculate(SageWorkspace *ws, float *error_host, const float *R10, const float *t10,
                                 const float *unscaled_dpts0, const float *matched_unscaled_dpts1, const float *homo0,
                                 const float *matched_homo1, float scale0, float scale1, float loss_param, float weight,
                                 int N);
int sage_tracker_match_geom_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host,
                                                const float *R, const float *t, const float *sampled_dpts0,
                                                const float *matched_dpts1, const float *homo0,
                                                const float *matched_homo1, float scale0, float loss_param,
                                                float weight, int with_scale, int N);
int sage_tracker_match_geom_error_calculate(SageWorkspace *ws, float *error_host, const float *R, const float *t,
                                            const float *sampled_dpts0, const float *matched_dpts1, const float *homo0,
                                            const float *matched_homo1, float loss_param, float weight, int N);

/* ---- f4 (matching core): descriptor response argmax with cycle consistency ------------------------------------------
 * Replaces the tensor expression of core/gtsam/match_geometry_factor.cpp:62-97 and
 * core/system/camera_tracker.cpp:608-633: for K keypoints of frame 0 (flat indices kp_loc1d_0, int64) the best match in
 * desc1 [C,H,W] under -sum_c (d0 - d1)^2, the best match of THAT descriptor back in desc0, and the inlier flag
 * |kp - cyc|_2 <= cyc_thresh (pixels).  The K x H*W response maps are never materialised.  Outputs are device arrays
 * of K entries; *n_inliers_host receives the number of flags set (synchronises).  The gather and the robust registration that
 * follow it: sage_match_points, sage_robust_registration above. */
int sage_cycle_match(SageWorkspace *ws, const float *desc0_dev, const float *desc1_dev, const int64_t *kp_loc1d_0,
                     int K, int C, int H, int W, float cyc_thresh, int64_t *raw_matched_loc1d_1,
                     int64_t *cyc_matched_loc1d_0, int32_t *inlier_flags, int *n_inliers_host);

/* ---- f1 producers: valid-pixel enumeration and seeded keyframe sampling ------------------------------------
 * sage_valid_locations: core/mapping/mapping_utils.h:254-287 (GenerateValidLocations): flat indices of mask > 0.5 in
 *   ascending order and their normalised homogeneous coordinates ((x-u0)/fx, (y-v0)/fy, 1).  Outputs are device
 *   arrays with room for H*W entries; *n_valid_host receives the count (synchronises the stream).
 * sage_shuffle_indices (host): the permutation mapper.cpp:1326-1333 draws -- std::iota, std::mt19937 seeded with
 *   (long)timestamp, std::shuffle -- through the same standard-library calls.
 * sage_sample_locations: mapper.cpp:1334-1340: the first min(num_samples, n_valid) shuffled indices gathered from the
 *   valid arrays into the keyframe's sampled_locations_1d / sampled_locations_homo.
 * sage_sort_locations (no reference counterpart): raster-orders a keyframe's sampled locations (and their homogeneous
 *   coordinates) out of place.  The factor sums do not depend on the order of the samples, the GPU's vector L1 does: on
 *   the shuffled list the reference keeps (mapper.cpp:1326-1340) the photometric kernels are 5-7x slower than on the
 *   sorted one.  The window engine (sage_window_finalize) does this internally; callers of the per-edge operators
 *   should sort once per keyframe.  *sorted_host = 0 (outputs = copy of the inputs) when a pixel is listed twice;
 *   SAGE_E_INVALID for a location outside H*W.  n = 0: *sorted_host = 1, the arrays may be NULL.  Synchronises the stream. */
int sage_sort_locations(SageWorkspace *ws, const int64_t *loc1d_dev, const float *homo_dev, int n, int H, int W,
                        int64_t *loc1d_out_dev, float *homo_out_dev, int *sorted_host);
int sage_valid_locations(SageWorkspace *ws, const float *mask_dev, const SageCamera *cam, int64_t *loc1d_dev,
                         float *homo_dev, int *n_valid_host);
int sage_shuffle_indices(int64_t seed, int64_t n, int64_t *idx_host);
int sage_sample_locations(SageWorkspace *ws, const int64_t *valid_loc1d_dev, const float *valid_homo_dev, int n_valid,
                          int64_t seed, int num_samples, int64_t *loc1d_dev, float *homo_dev, int *n_out_host);

/* sharded windows (sage_window_set_shard, world > 1): the in-place SUM all-reduce of a device buffer of n doubles
 * over all ranks, enqueued so that it is ordered with the window's stream (an RCCL ncclAllReduce on that stream, or
 * torch.distributed.all_reduce when the window runs on torch's current stream).  Returns 0 on success.  With the
 * hook installed sage_window_lm_step drives a sharded window as well: the host code between the launches stays
 * native.  Per iteration the hook is entered, in the classic sequence, once for the packed buffer and then once per
 * candidate evaluation for the 4-double error buffer; in the linearize-at-candidate sequence (the default of a reduced
 * window) once per evaluation for the candidate's packed buffer, after one more for the packed buffer at the current
 * estimate whenever that system has to be formed (the first iteration, after sage_window_reset); in the
 * domain-decomposed sequence once per evaluation for the separator buffer, followed by the 4-double error buffer when
 * the evaluation reaches the error pass.  (An evaluation whose host solve reports a non-positive pivot at once enters
 * it not at all.) */
typedef int (*SageAllReduceFn)(double *dev_buf, size_t n, void *user);
int sage_window_set_allreduce(SageWindow *w, SageAllReduceFn fn, void *user);

/* ---- domain-decomposed solve of a link-sharded window (host, double; csrc/shard_solve.cpp) ---------------------------
 * Link ranges are contiguous (sage_window_set_shard), so a rank's slice of the normal equations is complete for the
 * keyframes only its own links touch: it eliminates those locally (sage_shard_eliminate) and contributes the Schur
 * complement on the keyframes it shares with other ranks to the separator buffer -- the ONE all-reduced payload of an
 * LM iteration (sage_shard_sep_count doubles; 1.2 MB instead of the 3.0 MB packed system at K = 64 on 8 ranks).  After
 * the sum every rank factors the (identical) separator system and back-substitutes its own keyframes
 * (sage_shard_solve).  packed_local_host: this rank's UN-reduced packed normal equations in the layout of
 * sage_window_packed_dev; diag_add / g_add: the K*B diagonal priors of sage_block_solve, applied by the keyframe's
 * designated owner (the lowest rank touching it).  The separator buffer ends with 8 doubles: [0..3] the rank's error
 * / inlier totals at the linearisation point (tail of the packed buffer), [4..7] free for the caller (prior errors).
 * delta (K*B doubles): entries of the keyframes this rank touches are written, the others left alone.  B <= 40, as
 * for sage_block_solve: the plan constructors return SAGE_E_UNSUPPORTED above that. */
typedef struct SageShardPlan SageShardPlan;
int sage_shard_plan_create(int K, int nlinks, const int32_t *links, int B, int rank, int world, SageShardPlan **out);
void sage_shard_plan_destroy(SageShardPlan *p);
size_t sage_shard_sep_count(const SageShardPlan *p);
int sage_shard_num_separators(const SageShardPlan *p);
int sage_shard_num_interior(const SageShardPlan *p);
int sage_shard_keyframe_owner(const SageShardPlan *p, int kf);
int sage_shard_keyframe_is_local(const SageShardPlan *p, int kf);
int sage_shard_eliminate(SageShardPlan *p, const double *packed_local_host, double damp, const double *diag_add,
                         const double *g_add, double *sep_out);
int sage_shard_solve(SageShardPlan *p, const double *sep_reduced, double *delta);
/* The same decomposition inside ONE process: keyframe k belongs to domain k*ndomains/K, the newer endpoint of every
 * link that crosses a domain boundary is a separator (the first 3 keyframes of a domain in a temporal window, the far
 * end of a loop closure).  packed_host is then the ASSEMBLED system (domain 0 contributes the separator blocks).
 * sage_block_solve_domains = sage_block_solve computed that way on `ndomains` host threads: for long windows and for
 * loop closures, whose envelope rows would otherwise span the whole window. */
int sage_shard_plan_create_domains(int K, int nlinks, const int32_t *links, int B, int domain, int ndomains,
                                   SageShardPlan **out);
int sage_block_solve_domains(const double *packed_host, int K, int nlinks, const int32_t *links, int B, double damp,
                             const double *diag_add, const double *g_add, int ndomains, double *delta);

/* Native collective: RCCL (backend of record on MI355X: ring / tree over xGMI) bound at run time.  One process per GPU:
 *   rank 0:  sage_rccl_unique_id(id);   broadcast the 128 bytes by any means (MPI, a socket, torch.distributed);
 *   every rank, with its GPU current:   sage_rccl_comm_create(id, rank, world, &comm);
 *   sage_window_use_rccl(win, comm)     -> the window's two all-reduces per LM iteration become
 *        ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, comm, <the window's stream>)   -- no Python, no torch in the loop.
 * `comm` may equally be an ncclComm_t the host application already owns.  SAGE_E_UNSUPPORTED when no librccl is found. */
/* Development aid (bench.py --emulate-shard; csrc/window_dist.hip): adds the share of ranks that are not there after every
 * all-reduce of the window -- rest_dev = n_iterates packed systems (sage_window_packed_count doubles each, device memory,
 * kept alive by the caller), entry i evaluated at the i-th LM iterate since sage_window_reset.  One rank of an N-rank
 * job then walks the job's real trajectory on a one-GPU box with a one-rank communicator. */
int sage_window_emulate_peers(SageWindow *w, const double *rest_dev, int n_iterates);
#define SAGE_RCCL_ID_BYTES 128
int sage_rccl_unique_id(unsigned char *id128);
int sage_rccl_comm_create(const unsigned char *id128, int rank, int world, void **comm_out);
void sage_rccl_comm_destroy(void *comm);
/* what the communicator itself reports (ncclCommCount / ncclCommUserRank): bench.py prints it so that the first multi-GPU
 * line is self-verifying (r06) */
int sage_rccl_comm_info(void *comm, int *ranks_out, int *rank_out);
int sage_window_use_rccl(SageWindow *w, void *nccl_comm);

/* one full LM iteration: linearize -> (all-reduce) -> solve -> error at candidate -> (all-reduce) -> accept/reject
 * (policy of camera_tracker.cpp:1156-1279); windows that are reduced over ranks take the one-collective sequence
 * solve -> linearize at the candidate -> all-reduce -> accept/reject by themselves (SageLmConfig::linearize_at_candidate).
 * Sharded windows need sage_window_set_allreduce / sage_window_use_rccl first. */
typedef struct SageLmState
{
  double damp, error, candidate_error;
  int accepted, iters;
} SageLmState;
int sage_window_lm_step(SageWindow *w, SageLmState *st, const SageLmConfig *cfg);
/* n iterations of sage_window_lm_step in one call; trace (optional): n x {error, candidate_error, accepted, damp after the
 * step}; *done (optional) = iterations completed (an error code ends the run early). */
int sage_window_lm_run(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace, int *done);
/* the same + step_seconds[n]: host wall time of every iteration (entry of the call / return of the previous iteration ->
 * this iteration's accept / reject decision) */
int sage_window_lm_run_timed(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace, int *done,
                             double *step_seconds);
/* Sharded windows with the domain-decomposed solve (sage_shard_*: chosen at sage_window_finalize for world > 1 when
 * SAGE_SHARD_SCHUR=1, or by default from K >= 256 keyframes): sage_window_lm_step all-reduces the separator system
 * instead of the packed normal equations, and a rank only updates the keyframes its own links touch.  Call this (a
 * collective: every rank, through the window's all-reduce) before reading variables of other keyframes with
 * sage_window_get_keyframe; a no-op for windows that solve the whole system on every rank. */
int sage_window_sync_variables(SageWindow *w);

/* ---- Powell's dogleg, the optimiser the reference runs its graphs with (ISAM2 in Dogleg mode, initial radius 1.0,
 * ONE_STEP_PER_ITERATION: deepfactors.cpp:89, 397, 650, 1422).  DESIGN.md "Dogleg step" has the definitions.
 *
 * With A and g the window's system at damping 0 (diagonal blocks symmetrised, priors added, held rows the identity's with a
 * zero g entry), n = A^-1 g the Gauss-Newton point and u = (g.g / g.Ag) g the steepest-descent point, every trial point of
 * an iteration is  delta = a g + b n.  Six dot products determine its norm, its model decrease 2 g.delta - delta.A delta and
 * the blend: dots [6] = { g.g, g.n, n.n, g.Ag, g.An, n.An }. */
enum { SAGE_DOGLEG_SEARCH_EACH_ITERATION = 0, SAGE_DOGLEG_SEARCH_REDUCE_ONLY = 1, SAGE_DOGLEG_ONE_STEP_PER_ITERATION = 2 };
typedef struct SageDoglegConfig
{
  double init_delta; /* trust radius of the first iteration (1.0) */
  double min_delta;  /* the radius is halved only while it is above this (1e-5) */
  int mode;          /* SAGE_DOGLEG_*: how the radius is adapted (ONE_STEP_PER_ITERATION) */
} SageDoglegConfig;
void sage_dogleg_config_default(SageDoglegConfig *cfg);
/* carried from one iteration to the next: delta (<= 0 before the first iteration: cfg->init_delta is taken), solves, iters;
 * the rest describes the last iteration.  evals: error evaluations of the last iteration; solves: factorisations so far
 * (counted by the window step, one per iteration); accepted: 0 when the zero step was taken. */
typedef struct SageDoglegState
{
  double delta, error, candidate_error, rho, step_norm, sd_norm, gn_norm, a, b;
  double dots[6]; /* the dot products the last iteration was given */
  int region, accepted, evals, solves, iters;
} SageDoglegState;
/* The dogleg point for radius delta (ComputeDoglegPoint / ComputeBlend, DoglegOptimizerImpl.cpp:25-83) as the coefficients
 * of g and n; region: 0 steepest descent (u scaled to length delta), 1 blend, 2 Gauss-Newton.  g.g == 0: the zero step
 * (a = b = 0, region 0), SAGE_OK.  SAGE_E_NOT_PSD for g.Ag <= 0 (or NaN), SAGE_E_INVALID for a NULL output. */
int sage_dogleg_point(double delta, double gg, double gn, double nn, double gAg, double *a, double *b, int *region);
/* the error at x (+) (a g + b n) -> *f_candidate; a non-zero return ends the iteration with that code */
typedef int (*SageDoglegEvalFn)(void *ctx, double a, double b, double *f_candidate);
/* One iteration of the trust-region policy (DoglegOptimizerImpl::Iterate, DoglegOptimizerImpl.h:137-252) around `eval`:
 * gain ratio rho = (f_error - f_candidate) / model decrease, 0.5 when either decrease is below 1e-15 in magnitude;
 * rho >= 0.75: delta <- max(delta, 3 |step|); 0.25 <= rho < 0.75: delta kept; 0 <= rho < 0.25: delta halved while above
 * min_delta; rho < 0 or NaN: delta halved and the point evaluated again, at delta <= min_delta the zero step with the error
 * kept.  The search modes repeat the evaluation as Iterate does.  SAGE_E_INVALID for a NULL argument, SAGE_E_NOT_PSD as
 * sage_dogleg_point, otherwise what eval returned. */
int sage_dogleg_iterate(const SageDoglegConfig *cfg, const double *dots, double f_error, SageDoglegEvalFn eval, void *ctx,
                        SageDoglegState *st);
/* Per keyframe the blocks of the packed buffer its rows of A v are summed from, in the order they are summed: the diagonal
 * block first, then the links in the order they were added (duplicates and hubs included).  links [nlinks][2];
 * offsets [K + 1]; entries [K + 2 nlinks][2] = (block: k or K + link, transposed: 0 for the link's first keyframe, whose
 * rows the block holds, 1 for its second).  SAGE_E_INVALID for NULL, K < 1, nlinks < 0, an end outside [0, K) or a == b. */
int sage_dogleg_incidence(int K, int nlinks, const int32_t *links, int32_t *offsets, int32_t *entries);

/* One dogleg iteration on a finalized single-rank window with the device solver: linearize at the current estimate, ONE
 * solve at damping 0, the products, sage_dogleg_iterate around the candidate kernel and the error pass, accept or keep.
 * st->solves rises by one per call whatever st->evals is.  SAGE_E_NOT_PSD (window and st unchanged) for a non-positive
 * pivot of the Gauss-Newton factorisation -- the caller may take an LM step instead (gtsam throws).  SAGE_E_UNSUPPORTED for
 * sharded or reduced windows and windows without a device solver (duplicate links); SAGE_E_STATE before finalize;
 * SAGE_E_INVALID for NULL. */
int sage_window_dogleg_step(SageWindow *w, SageDoglegState *st, const SageDoglegConfig *cfg);
/* n steps; trace (optional): n x {error, candidate_error, accepted, delta after the step, rho, region, evals}; *done
 * (optional) = steps completed (an error code ends the run early). */
int sage_window_dogleg_run(SageWindow *w, SageDoglegState *st, const SageDoglegConfig *cfg, int n, double *trace, int *done);
/* The primitives behind the step.  _products: valid after a linearize and a sage_window_solve at damping 0; Ag and An in
 * one pass over the packed buffer, then dots [6] (two runs agree in every bit).  _candidate: the candidate variables and
 * their host mirrors for delta = a g + b n, exactly what the solve's retraction leaves for the same delta (so
 * sage_window_accept, sage_window_get_delta and the error pass work unchanged); valid after _products.
 * _get_dogleg_vectors: host copies of the last _products call's vectors (a step's included), K * B doubles each, any may
 * be NULL. */
int sage_window_dogleg_products(SageWindow *w, double *dots);
int sage_window_dogleg_candidate(SageWindow *w, double a, double b);
int sage_window_get_dogleg_vectors(SageWindow *w, double *g, double *Ag, double *n, double *An);

/* Partial relinearization, as ISAM2 relinearizes (cacheLinearizedFactors, relinearizeSkip 1, per-key thresholds:
 * core/deepfactors.cpp:1421-1437; ISAM2-impl.h:345-372): only the factors that touch a key whose linearization point moved
 * are linearized again, every other factor keeps its cached HessianFactor.
 *
 * Who reads what.  A directed edge a -> b (source a; numbered as sage_window_get_edge numbers them) reads
 *     photometric   pose a, pose b, code a, scale a      the depth map of a
 *     geometric     pose, code and scale of both         the depth maps of a and b, the gradient of b's
 * so a change of code b alone leaves the photometric edge a -> b clean.  "Changed" = the float bits differ (the memcmp of
 * sage_window_prepass: -0.0f against 0.0f is a change).
 *
 * sage_relin_plan (host only, stateless): the reads table applied to two variable sets.  links [n_links][2] (either order of
 * a link's keyframes; direction 0 starts at the lower one), pose [K][12], code [K][CS], scale [K]; photo_stale, geo_stale
 * [2 * n_links]: 1 for a directed edge of that type that reads a changed group; map_read [K]: 1 for a keyframe whose depth
 * map a stale edge reads; n_photo, n_geo (optional): the numbers of stale edges.  SAGE_E_INVALID for a NULL array, K < 1,
 * CS < 1, n_links < 0, a link end outside [0, K) or a link of a keyframe with itself.
 *
 * sage_window_set_relinearization (after finalize, SAGE_E_STATE before; SAGE_E_INVALID for another mode; SAGE_E_UNSUPPORTED
 * for SAGE_RELIN_STALE on a sharded window): in SAGE_RELIN_STALE sage_window_linearize -- and with it a linearizing
 * sage_window_prepass -- launches only the dense edges whose inputs differ from the values their device-resident result was
 * computed at, byte for byte what SAGE_RELIN_ALL (the default) computes for them; the other edges keep their results,
 * {error, inliers} included: an error pass at other values in between does not touch them.  Depth maps are rebuilt only
 * for the keyframes a launched edge reads, and only when they were built from other code / scale bits.  The keypoint and
 * graph terms are evaluated in full every time (one launch per group of at most 512 points each: launch latency, and
 * bit-identical anyway), and so is the assembly.  Nothing stale: no dense launch; the values and the packed system both
 * current: nothing is launched at all.  Every edge is stale after a switch of the mode, sage_window_lm_step and the dogleg
 * step (their merged linearize leaves mixed results), sage_window_set_runs / sage_window_tune_runs and sage_window_reset.
 * The error pass stays whole-window.
 * In SAGE_RELIN_STALE a recomputing sage_window_prepass copies only the re-evaluated edges' AtA / Atb rows to the host
 * cache (the term groups in full) and keeps the clean edges' rows across an error-only prepass at other values.
 *
 * sage_window_last_evaluation: what the last sage_window_linearize (either mode) evaluated: dense edges and work items per
 * factor type, depth maps and gradient maps built, and the AtA / Atb rows a prepass around it copied to the host. */
enum { SAGE_RELIN_ALL = 0, SAGE_RELIN_STALE = 1 };
typedef struct SageEvalCounts
{
  int32_t photo_edges, geo_edges, depth_maps, depth_grads, photo_items, geo_items, host_entries_pulled;
} SageEvalCounts;
int sage_relin_plan(int K, int CS, int n_links, const int32_t *links, const float *pose_old, const float *code_old,
                    const float *scale_old, const float *pose_new, const float *code_new, const float *scale_new,
                    uint8_t *photo_stale, uint8_t *geo_stale, uint8_t *map_read, int32_t *n_photo, int32_t *n_geo);
int sage_window_set_relinearization(SageWindow *w, int mode);
int sage_window_last_evaluation(const SageWindow *w, SageEvalCounts *out);
/* The relinearization check and the masked accept: with them a window runs ISAM2's fluid loop -- linearize (stale),
 * sage_window_solve or a dogleg point, marks, masked accept -- where every factor is linearized at the current point and
 * only the work is partial.
 * sage_relin_marks (host only, stateless): gtsam's CheckRelinearizationFull with per-key vector thresholds.  delta [K][7+CS]
 * in the window's block order (pose 6, code CS, scale); marks [K]: the SAGE_HOLD_* bits of the groups with any
 * |delta_i| > threshold_i (strictly; a NaN marks nothing); n_marked (optional): the number of groups marked.
 * SAGE_E_INVALID for a NULL delta, t or marks, K < 1, CS < 1.
 * sage_window_relin_marks: the same on the last solve's delta (sage_window_get_delta), with the groups held by
 * sage_window_hold cleared (gtsam erases fixedVariables).  SAGE_E_STATE before finalize.
 * sage_window_accept_marked: candidate -> current for the marked groups only (ISAM2's ExpmapMasked: the candidate is the
 * retraction of the last solve's delta); unmarked groups keep their linearization point, held groups are never moved.  The
 * candidate set becomes the new current set as well.  SAGE_E_INVALID for NULL or bits outside SAGE_HOLD_*; SAGE_E_STATE
 * before finalize. */
typedef struct SageRelinThresholds
{
  float pose[6];
  float code;
  float scale;
} SageRelinThresholds;
int sage_relin_marks(const double *delta, int K, int CS, const SageRelinThresholds *t, int32_t *marks, int32_t *n_marked);
int sage_window_relin_marks(const SageWindow *w, const SageRelinThresholds *t, int32_t *marks, int32_t *n_marked);
int sage_window_accept_marked(SageWindow *w, const int32_t *marks);

/* =====================================================================
 * Prepared keyframes: a keyframe's pose-independent preparation, done once and shared between windows
 * =====================================================================
 * sage_window_finalize prepares every keyframe it was given as a view: the channel-group relay of its pyramids with the level's
 * focal lengths and sqrt(w_l) folded in, its sampled locations validated and relaid in 8 x 8 tile order (tile-padded where that
 * is cheap), its pre-sampled source features.  None of that depends on a pose, a code, a scale, a link or on who else is in
 * the window, and the mapper builds a window per new keyframe over keyframes it has seen before.  A SagePreparedKeyframe holds
 * that preparation; any number of windows borrow it, in any mix with views, and skip those stages for it.
 *
 * A prepare call reads pyr, FS and photo_weights from cfg, nothing else, and the process's SAGE_SAMPLE_TILE / SAGE_SAMPLE_PAD
 * switches as finalize does; the handle records all of them.  It OWNS the relaid planes, the ordered sample arrays and the
 * pre-sampled features (one device allocation, sized from N before any launch: cap = max(1, ceil(5 N / 4)) sample slots --
 * the padded order is only ever chosen at slots <= 1.25 N) and BORROWS the view's feat_pyr, grad_pyr, bias, basis, loc1d and
 * homo, which must outlive the handle as they must outlive a window (the texture-path sampler and an unordered keyframe
 * still read them).  The handle is immutable once the call returns, and the call returns with the workspace's stream
 * synchronised: any window on any stream or host thread of the SAME DEVICE may take it -- a handle belongs to the device it
 * was prepared on.  The reference count is atomic: the caller's reference, one per window that holds the handle
 * (sage_window_add_prepared_keyframe retains; sage_window_destroy releases); the last release frees.
 *
 * sage_keyframe_prepare_batch: B keyframes in launches that do not depend on B -- one relay kernel over all 3 B planes, the
 * batched location sort (two fills, mark, order), one wait for status and tile counts, a second ordering pass and wait only
 * if some keyframe takes the padded order, one pre-sampling kernel, the final wait: 6 launches and 2 waits, or 7 and 3.
 * sage_keyframe_prepare is the batch of one.  SAGE_E_INVALID, and no handle left behind (every out[b] NULL): a NULL
 * argument or view pointer, N < 0, B < 1, B > SAGE_PREPARE_MAX_BATCH, FS % 4 != 0 or FS < 4, a pyramid of no or too many
 * levels, a negative or NaN level weight, a location outside the image.
 * sage_keyframe_prepare_plan (host only; every output pointer may be NULL): per keyframe the bytes of its allocation, the
 * bytes of the call's scratch on the workspace, and the launches and waits of a batch without a padded keyframe.
 * sage_keyframe_prepare_launches: what the last prepare call on ws launched.
 * sage_keyframe_config_matches: 1 when two configurations prepare a keyframe alike -- pyr, FS and photo_weights bit for bit
 * -- else 0; the comparison sage_window_add_prepared_keyframe makes between the handle's record and its window.
 * sage_keyframe_get (parity tests; synchronises the device): SAGE_PREP_PACKED the three relaid planes [3][FS/4][P][4] floats,
 * SAGE_PREP_LOC the `slots` int64 locations, SAGE_PREP_HOMO the [slots][3] rays, SAGE_PREP_F0S the [L][FS/4][slots][4]
 * pre-sampled floats; `bytes` must be the array's size.  Of a keyframe with ordered == 0 LOC and HOMO are the caller's.
 *
 * sage_window_add_prepared_keyframe: as sage_window_add_keyframe, the keyframe id.  SAGE_E_STATE after finalize, SAGE_E_INVALID
 * for NULL and for a handle whose recorded pyr / FS / photo_weights / sample switches are not bit-equal to the window's.
 * Stages 3-5 of finalize then run for the views only (a window without views launches nothing there); nothing else in the
 * window notices the difference, and a window built from handles computes bit for bit what its twin from views computes.
 * sage_window_build_stats: what stages 3-5 of the last finalize did. */
typedef struct SagePreparedKeyframe SagePreparedKeyframe;
#define SAGE_PREPARE_MAX_BATCH 64           /* the headline window in one call */
enum { SAGE_PREP_PACKED = 0, SAGE_PREP_LOC = 1, SAGE_PREP_HOMO = 2, SAGE_PREP_F0S = 3 };

typedef struct SagePreparedInfo {           /* host */
  int32_t N;            /* the caller's samples                                             */
  int32_t slots;        /* what a window's kernels walk: N, or 64 * tiles when padded       */
  int32_t ordered;      /* 0: a pixel was sampled twice, the caller's order and arrays are kept */
  int32_t padded;       /* 1: tile-padded order (holes = location -1, ray (0,0,1))          */
  int32_t refs;         /* the caller's reference + one per window that holds it            */
  uint64_t device_bytes;
} SagePreparedInfo;

int  sage_keyframe_prepare(SageWorkspace *ws, const SageWindowConfig *cfg, const SageKeyframeView *view,
                           SagePreparedKeyframe **out);
int  sage_keyframe_prepare_batch(SageWorkspace *ws, const SageWindowConfig *cfg, const SageKeyframeView *views, int B,
                                 SagePreparedKeyframe **out /* [B] */);
int  sage_keyframe_prepare_plan(const SageWindowConfig *cfg, const int32_t *N /* [B] */, int B,
                                uint64_t *device_bytes /* [B] */, uint64_t *scratch_bytes, int *launches, int *waits);
int  sage_keyframe_prepare_launches(const SageWorkspace *ws);   /* of the last prepare call on ws */
int  sage_keyframe_config_matches(const SageWindowConfig *a, const SageWindowConfig *b);
int  sage_keyframe_info(const SagePreparedKeyframe *pk, SagePreparedInfo *out);
int  sage_keyframe_get(const SagePreparedKeyframe *pk, int what, void *host, size_t bytes);   /* parity tests */
void sage_keyframe_release(SagePreparedKeyframe *pk);            /* NULL: no-op */

int  sage_window_add_prepared_keyframe(SageWindow *w, SagePreparedKeyframe *pk, const float *pose12,
                                       const float *code, float scale);   /* returns the keyframe id, as add_keyframe */
typedef struct SageWindowBuildStats { int32_t keyframes, prepared, repacked, ordered, presampled, launches; } SageWindowBuildStats;
int  sage_window_build_stats(const SageWindow *w, SageWindowBuildStats *out);   /* stages 3-5 of the last finalize */

/* ---- f7: marginal priors -- a sliding window as a fixed-lag smoother ------------------------------------------------
 * No reference counterpart (its MarginalizeFrames is commented out; ISAM2 keeps every factor).  When a window slides, the
 * keyframes that leave are marginalised: their factors, linearised at the window's current variables, are eliminated by a
 * Schur complement into a dense Gaussian prior over the keyframes they were linked to, and the next window carries that
 * prior as one more term.
 *
 * Convention (the window's): e(d) = e - 2 g^T d + d^T A d, step A d = g.  A prior over m keyframes holds Lambda [mB x mB],
 * eta [mB], c (B = 7 + CS; rows per keyframe: pose 6, code CS, scale 1) and the linearisation point of its keyframes.  At
 * variables x its term is   AtA = Lambda (constant: first-estimate Jacobians, the linear-container treatment),
 * Atb = eta - Lambda delta,   err = delta^T Lambda delta - 2 eta^T delta + c,   with
 * delta_k = [pose_local(x0_k, x_k) (6), code - code0 (CS), scale - scale0 (1)].  pose_local(x, x) is not exactly zero in
 * translation (fp32 rotation matrices are not exactly orthonormal): nothing here is bit-exact zero at the linearisation point.
 *
 * sage_schur_marginal (host, fp64): A [n x n] (symmetrised as (A + A^T) / 2 on the way in), g [n], e, and the rows to drop
 * (distinct; the keep rows are the others, ascending) ->
 *   Lambda = A_kk - A_kd A_dd^-1 A_dk (symmetrised exactly), eta = g_k - A_kd A_dd^-1 g_d, c = e - g_d^T A_dd^-1 g_d.
 * Cholesky of A_dd: SAGE_E_NOT_PSD for a non-positive pivot, nothing written.  A drop row that is a row of the identity with a
 * zero gradient (a held variable: sage_window_hold) eliminates to nothing.  n_drop = 0 is allowed, n_drop = n is not.
 *
 * SageMarginalPrior: opaque host handle.  _create copies the arrays (kf_ids NULL: 0 .. m-1); SAGE_E_UNSUPPORTED for m > 16
 * (SAGE_PRIOR_MAX_KEYFRAMES) or a CS the window engine does not instantiate.  _get / _keyframes: any output of _get may be
 * NULL.  _destroy(NULL) is a no-op.
 * sage_prior_evaluate: host mirror of the device term at the given variables of the prior's m keyframes (pose12 [m][12],
 * code [m][CS], scale [m]): delta [mB], Atb [mB], err, each optional.
 * sage_prior_term_plan (host, tests): the terms of n_terms priors (m [n_terms]; kf_maps: their maps one behind the other)
 * added in order to a window of K keyframes and `links` [nlinks][2] -> the structure-only links appended (append [.][2],
 * room for sum m (m - 1) / 2) and where every block (i <= j) of every Lambda lands on `rank`: place [.][5] = term, i, j,
 * packed block (keyframe id, or K + link), transposed (room for sum m (m + 1) / 2; ascending packed block, then term id);
 * owned [n_terms]: 1 on rank 0, 0 elsewhere.  Refusals as sage_window_add_prior_term's. */
#define SAGE_PRIOR_MAX_KEYFRAMES 16
typedef struct SageMarginalPrior SageMarginalPrior;
int  sage_schur_marginal(const double *A, const double *g, double e, int n, const int32_t *drop, int n_drop, double *Lambda,
                         double *eta, double *c);
int  sage_marginal_prior_create(int m, int CS, const double *Lambda, const double *eta, double c, const float *pose12,
                                const float *code, const float *scale, const int32_t *kf_ids, SageMarginalPrior **out);
int  sage_marginal_prior_dims(const SageMarginalPrior *p, int *m, int *CS);
int  sage_marginal_prior_get(const SageMarginalPrior *p, double *Lambda, double *eta, double *c, float *pose12, float *code,
                             float *scale);
int  sage_marginal_prior_keyframes(const SageMarginalPrior *p, int32_t *kf_ids /* [m] */);
void sage_marginal_prior_destroy(SageMarginalPrior *p);
int  sage_prior_evaluate(const SageMarginalPrior *p, const float *pose12, const float *code, const float *scale, double *delta,
                         double *Atb, double *err);
int  sage_prior_term_plan(int K, int nlinks, const int32_t *links, int n_terms, const int32_t *m, const int32_t *kf_maps,
                          int rank, int world, int32_t *append, int32_t *n_append, int32_t *place, int32_t *n_place,
                          int32_t *owned);
/* sage_window_add_prior_term: a third family of terms next to the keypoint and graph terms.  Before finalize (SAGE_E_STATE
 * afterwards).  kf_map [m]: the keyframes of THIS window the prior's rows belong to, distinct and valid, any order
 * (SAGE_E_INVALID otherwise, or for a prior of another CS).  The prior is copied: the handle may be destroyed.  Every pair of
 * the prior's keyframes needs a link block: for a pair without a link the call appends a structure-only link (what
 * sage_window_add_keypoint_link creates), in ascending (a, b) order -- link ids handed out afterwards move on by that many.
 * Returns the term id.  A sharded window gives every prior term to rank 0 (like a scale-prior graph term); a window of the
 * domain-decomposed solve answers SAGE_E_UNSUPPORTED at finalize.
 * The term is evaluated on every linearize and every error pass (prior_eval_kernel; prior_add_kernel adds Lambda, unrounded,
 * the Atb rows and the error -- in the geometric error slot, where graph terms ride -- to the packed system behind the
 * assembly).  No atomics: bit-reproducible from run to run.  The gtsam factor cache, SAGE_RELIN_STALE and SageEvalCounts
 * know nothing of the family.  Profiler slots (sage_window_get_kernel_time): 8 prior_eval_kernel, 9 prior_add_kernel.
 * sage_window_get_prior_term: host copy of the last linearize in doubles, AtA [mB x mB] (= Lambda), Atb [mB], err; each
 * optional.  SAGE_E_STATE before the first linearize, SAGE_E_INVALID for a term of another rank. */
int  sage_window_add_prior_term(SageWindow *w, const SageMarginalPrior *prior, const int32_t *kf_map /* [m] */);
int  sage_window_num_prior_terms(const SageWindow *w);
int  sage_window_get_prior_term(const SageWindow *w, int term, double *AtA, double *Atb, double *err);
/* sage_window_marginalize: the prior the keyframes drop [n_drop] leave behind.  The window must hold a linearization at its
 * current variables (sage_window_linearize, or an accepted linearize-at-candidate step): SAGE_E_STATE otherwise, as
 * sage_window_solve after sage_window_set_runs.  The sub-system is the sum, in double, of exactly the fp32 per-edge and
 * per-term results that linearize left, placed by the assembly's rules, of ONLY the factors incident to a dropped keyframe:
 * the dense edges of both directions and factor types, the keypoint and graph terms on those edges, a scale-prior graph term
 * on a dropped keyframe, the dropped keyframes' own diagonal priors (code prior; keyframe 0's scale and pose priors), and
 * every prior term that touches a dropped keyframe, whole.  Factors between two surviving keyframes do not enter: they stay
 * in the next window.  The separator -- the prior's keyframes, sage_marginal_prior_keyframes -- is every surviving keyframe
 * that shares a link or a prior term with a dropped one, ascending.  The hold rule is applied before the elimination: a held
 * row of a dropped keyframe is a row of the identity, a held row of a separator keyframe a zero row of Lambda and eta.  The
 * linearisation point is the window's current variables.  c counts the dropped keyframes' diagonal priors as
 * sage_window_total_error counts them.
 * SAGE_E_INVALID: a bad or duplicate id, dropping every keyframe, or dropped keyframes nothing links to a survivor;
 * SAGE_E_UNSUPPORTED: a sharded window (world > 1: no rank holds every result), or a separator of more than 16 keyframes;
 * SAGE_E_NOT_PSD: the dropped keyframes' block is not positive definite. */
int  sage_window_marginalize(SageWindow *w, const int32_t *drop, int n_drop, SageMarginalPrior **out);

/* ---- marginal covariances (covariance_host.cpp, window_covariance.hip, depth_sigma.hip) ----
 * How certain a window's estimate is: the blocks of Sigma = M^-1 for every keyframe and every linked pair, what gtsam hands
 * back as ISAM2::marginalCovariance / Marginals.  M = L L^T is the block Cholesky factor a solve leaves on the host; the
 * blocks of Sigma on the factor's pattern are one backward recursion over it (selected inverse), no second factorisation:
 *   Sigma_ij = -(sum_{k in col(j)} Sigma_ik L_kj) L_jj^-1,   Sigma_jj = (L_jj^-T - sum_k Sigma_jk L_kj) L_jj^-1, symmetrised
 * exactly.  One thread, one fixed order: the result is the same bit for bit from run to run.
 *
 * sage_block_covariance (host, fp64), the sibling of sage_block_solve: the same damped matrix
 * (H + diag_add) + damp diag(H + diag_add) of a packed buffer (the gradient is not read), duplicate links summed.
 * pairs [n_pairs][2]: (a, a) asks for a keyframe's diagonal block, (a, b) for a link's block, either way round: (b, a) is the
 * transpose of (a, b) bit for bit; SAGE_E_INVALID for a pair that is not a link.  Sigma [n_pairs][B*B] row-major, rows of
 * pairs[.][0], columns of pairs[.][1].  SAGE_E_NOT_PSD as the solve answers it, nothing written; SAGE_E_UNSUPPORTED for B > 40.
 * sage_covariance_plan (host, tests): the blocks (lower triangle with the diagonal) the elimination plan of K keyframes and
 * `links` stores, and how many the recursion's symbolic closure adds to them (none for the plans in use).
 *
 * sage_window_covariance: drains the stream and runs the recursion on the factor the window's last successful solve left
 * (sage_window_solve, sage_window_lm_step, a dogleg solve); damp_out (optional) receives that solve's damping.  At damping 0
 * -- after the dogleg's solve or sage_window_solve(w, 0, ..) -- Sigma is A^-1 of the system with its diagonal priors, keypoint,
 * graph and prior terms: what ISAM2::marginalCovariance returns when the factors are served as sage_window_factor serves
 * them (G = AtA).  With damping it is the inverse of the DAMPED system, a lower bound of that.  Sigma belongs to the
 * linearization it was solved at: a later solve invalidates it, a later linearize or accept does not.
 * SAGE_E_STATE before the first solve, after a solve that failed and after whatever drops the system (sage_window_tune_runs,
 * sage_window_set_runs); SAGE_E_UNSUPPORTED for a sharded window (world > 1: as sage_window_marginalize), a window of the
 * domain-decomposed solve and a window without a device solver (duplicate links).
 * sage_window_get_covariance: block (kf_a, kf_b) of the stored Sigma, [B*B] row-major, rows of kf_a, in the window's row
 * order [pose 6, code CS, scale]: kf_a == kf_b or a link (structure-only links included), either way round.  Held rows and
 * columns are exactly 0, and so are the rows of a group that left the solver (sage_window_solver_block_size < B): a held
 * variable has no variance.  SAGE_E_STATE without a stored Sigma, SAGE_E_INVALID for a pair without a link block.
 *
 * Depth uncertainty: d(p) = s (bias(p) + basis(p,:) code) has the Jacobian j = [s basis(p,:) (CS), bias(p) + basis(p,:) code]
 * against (code, scale); with S the (code, scale) sub-block of Sigma_kk, [(CS+1) x (CS+1)],
 *   var(p) = j^T S j,   sigma(p) = sqrtf(max(var, 0)).
 * sage_depth_sigma_batch: n keyframes in one launch (depth_sigma_kernel: pixel tiles x keyframes, S staged in LDS, fp32, no
 * atomics, a fixed summation order: bit-reproducible), asynchronous on the workspace's stream like sage_depth_and_grad.  S is
 * read from the HOST by the call, symmetrised as (S + S^T) / 2 and rounded once to fp32.  CS 16 or 32 (SAGE_E_UNSUPPORTED
 * otherwise), mode SAGE_DEPTH_VARIANCE or SAGE_DEPTH_SIGMA; argument checks come before any launch.
 * sage_window_depth_sigma: the same launch on the window's stream for the keyframes kfs [n], with bias, basis, code and scale
 * of the window's own depth table at the current variables (prepared keyframes included) and S from the stored Sigma:
 * SAGE_E_STATE without one.  out_dev [n] -> [H*W] device floats.  A keyframe whose code and scale are held gives zeros.
 * sage_window_depth_sigma_timing (scripts/covariance_bench.py): the sigma kernel over all K keyframes and depth_batch_kernel
 * over the same keyframes, alternating, reps times each between HIP events on the window's stream -> the medians in
 * microseconds.  It leaves the depth maps of the current variables behind, as an error pass at them would. */
enum { SAGE_DEPTH_VARIANCE = 0, SAGE_DEPTH_SIGMA = 1 };
typedef struct SageDepthSigmaItem
{
  const float *bias_dev, *basis_dev, *code_dev; /* [H*W], [H*W,CS], [CS] */
  float scale;
  const double *cov_code_scale;                 /* HOST, [CS+1][CS+1] */
  float *out_dev;                               /* [H*W] */
} SageDepthSigmaItem;
int  sage_block_covariance(const double *packed_host, int K, int nlinks, const int32_t *links, int B, double damp,
                           const double *diag_add, const int32_t *pairs /* [n_pairs][2] */, int n_pairs, double *Sigma);
int  sage_covariance_plan(int K, int nlinks, const int32_t *links, int32_t *stored, int32_t *added);
int  sage_window_covariance(SageWindow *w, double *damp_out);
int  sage_window_get_covariance(const SageWindow *w, int kf_a, int kf_b, double *Sigma /* [B*B] */);
int  sage_depth_sigma_batch(SageWorkspace *ws, const SageDepthSigmaItem *items, int n, int H, int W, int CS, int mode);
int  sage_window_depth_sigma(SageWindow *w, const int32_t *kfs, int n, int mode, float *const *out_dev);
int  sage_window_depth_sigma_timing(SageWindow *w, int mode, int reps, double *sigma_us, double *depth_batch_us);

/* ---- TSDF fusion (tsdf_host.cpp, tsdf.hip, window_tsdf.hip) ----
 * The stage that turns keyframe depth maps, poses and a per-pixel std image into the fused surface: TSDFVolume.integrate of
 * representation/scripts/generate_reconstruction_fly_through.py:130-331 (a kernel kept as a string there).  The reference has
 * no uncertainty to give it and fills the std image with ones (:601-606); a window hands it its depth sigma maps.
 *
 * The volume: dim = (dx, dy, dz) voxels in C order [x][y][z], z fastest; tsdf, weight and (optional) color, fp32, zero at
 * creation; origin fp32 x 3; voxel_size and trunc_margin fp32.
 * One view (a depth image with its pose): for every voxel (ix, iy, iz), in fp32, one operation at a time, NO fused
 * multiply-add, division correctly rounded:
 *   1. p = origin + (float)i * voxel_size                       (one multiply, then one add, per axis)
 *   2. q = p - t                                                (pose12 = [R row-major, t], world from camera)
 *   3. c_x = (R[0][0] q_x + R[1][0] q_y) + R[2][0] q_z, c_y and c_z with columns 1 and 2   (R^T q, summed left to right)
 *   4. skip if c_z < min_depth
 *   5. u = (int)roundf(fx (c_x / c_z) + cx), v likewise; roundf rounds half away from zero (-0.4 is pixel 0, inside)
 *   6. skip if u < 0, u >= w, v < 0 or v >= h
 *   7. d = depth[v w + u] (0 where mask[v w + u] <= 0.5), s = std[v w + u] (1 without a std image), s = fmaxf(s, std_floor);
 *      skip if d <= 0 or s <= 0
 *   8. diff = d - c_z; skip if diff < -trunc_margin
 *   9. dist = fminf(1, diff / s)                                (clipped above only: the lower end is -trunc_margin / s)
 *  10. w_new = w_old + obs_weight; tsdf = (tsdf w_old + dist obs_weight) / w_new; weight = w_new
 *  11. with a color image (packed b 65536 + g 256 + r in one float): old and new unpacked with floorf, every channel
 *      fminf(roundf((old w_old + new obs_weight) / w_new), 255), repacked
 * The running average does not commute in floating point: the order of the views is part of the result.
 * Where this departs from the reference's text: (i) the voxel's coordinates come from the linear index by integer arithmetic
 * (the reference divides in fp32, which is wrong above 2^24 voxels, and lets index N through); (ii) the reference's bits
 * depend on nvcc's contraction, these are the operations as written; (iii) the unused uncertainty volume does not exist;
 * (iv) a pixel coordinate that is NaN (0 / 0: possible only with min_depth <= 0) skips the voxel.
 * With sigma maps as the std image a voxel's value is sum_i w_i (d_i - z) / s_i / sum_i w_i wherever no view clips: its zero
 * crossing lies at the inverse-sigma-weighted mean depth sum_i (d_i / s_i) / sum_i (1 / s_i).
 *
 * Host planning (no device):
 * sage_tsdf_frustum_bounds: get_view_frustum (:376-387) folded into the running minimum / maximum of :561-567.  Five points in
 * double -- the camera centre and the image corners (0 | w, 0 | h) at max_depth, as ((u - cx) max_depth) / fx -- taken to
 * world coordinates and folded into bounds = [min x, y, z, max x, y, z], which the CALLER initialises: zeros reproduce the
 * script, whose volume therefore always contains the world origin; the first view's own points can be had with +-infinity.
 * SAGE_E_INVALID for NULL, fx or fy not positive, w or h < 1, a pose or max_depth that is not finite.
 * sage_tsdf_plan: voxel = base_voxel cbrt(prod((max - min) / base_voxel) / max_voxels) (:569-574, applied always, as the
 * script does; max_voxels <= 0 keeps base_voxel), dim = ceil((max - min) / voxel) (:138-141), origin = (float)min,
 * trunc_margin = voxel trunc_multiplier.  device_bytes: the volume's arrays and its per-brick counts.  SAGE_E_INVALID for
 * NULL, bounds that are empty along an axis or not finite, base_voxel or trunc_multiplier not positive and finite, and a
 * voxel count above 2^31 - 1.
 *
 * sage_tsdf_create / _destroy / _reset (zeros, on the stream) / _get (host copies, any may be NULL; drains the stream) /
 * _dev (the device arrays; color NULL for a volume without one).  The volume lives on its workspace's stream and must be
 * destroyed before the workspace.
 * sage_tsdf_integrate: one view, one launch (tsdf_integrate_kernel: one thread per voxel, lanes along z), asynchronous on the
 * workspace's stream: the view's device arrays must stay valid until the stream has passed the call.  A view with a color
 * image on a volume without a color array: SAGE_E_INVALID.  Argument checks come before any launch.
 * sage_tsdf_integrate_batch: n views (1 <= n <= SAGE_TSDF_MAX_VIEWS) in ONE launch, whatever n
 * (sage_tsdf_integrate_batch_launches).  Contract: the volume afterwards equals, byte for byte, n calls of sage_tsdf_integrate
 * in the order given.  A workgroup owns a brick of voxels (its long side, 64, along z), keeps their tsdf, weight and color in
 * registers while it walks the views in order and writes them once: the volume crosses HBM once, not n times.  The views'
 * parameters are uploaded once and staged in LDS sage_tsdf_view_chunk() at a time; before it walks a chunk the workgroup
 * drops the views none of its voxels can pass steps 4-6 of (the brick's eight corners against the four side planes and the
 * min_depth plane, with a slack for the fp32 rounding: DESIGN.md s3).  The cull only removes work whose outcome is "skip":
 * SAGE_TSDF_NO_CULL keeps every view and gives the same bytes.  SAGE_TSDF_BRICK_X1 / _X2 / _X4 choose the brick's extent
 * along x (voxels per thread) for measurements; 0 is the shape in use.  No atomics, every output has one writer.
 * sage_tsdf_last_stats: drains the stream and sums the per-brick counts of the last batch. */
#define SAGE_TSDF_MAX_VIEWS 1024
enum { SAGE_TSDF_NO_CULL = 1, SAGE_TSDF_BRICK_X1 = 1 << 4, SAGE_TSDF_BRICK_X2 = 2 << 4, SAGE_TSDF_BRICK_X4 = 3 << 4 };
enum { SAGE_TSDF_STD_ONE = 0, SAGE_TSDF_STD_SIGMA = 1 };
typedef struct SageTsdfPlan
{
  int32_t dim[3];
  int32_t with_color;
  float origin[3];
  float voxel_size, trunc_margin;
  int64_t voxels;       /* dim[0] dim[1] dim[2] */
  int64_t device_bytes;
} SageTsdfPlan;
typedef struct SageTsdfView
{
  const float *depth_dev;  /* [h*w], required */
  const float *std_dev;    /* [h*w], or NULL: 1 wherever depth > 0 (the script's ones * valid_mask) */
  const float *mask_dev;   /* [h*w], or NULL: no mask; a pixel with mask <= 0.5 reads depth 0 (the script's depth_map * mask) */
  const float *color_dev;  /* [h*w] packed, or NULL: the color volume is not touched */
  int64_t image_floats;    /* the floats every image above holds: fewer than cam.w * cam.h is SAGE_E_INVALID */
  float pose12[SAGE_POSE_FLOATS]; /* world from camera */
  SageCamera cam;
  float obs_weight, min_depth;
  float std_floor;         /* s = fmaxf(s, std_floor) before the s <= 0 test; 0: the reference's rule.  A held keyframe's
                              sigma map is exactly 0 and would otherwise contribute nothing */
} SageTsdfView;
typedef struct SageTsdfStats
{
  int64_t bricks, pairs, pairs_kept; /* pairs = bricks * views */
  int32_t views, brick[3];
} SageTsdfStats;
typedef struct SageTsdfVolume SageTsdfVolume;
int  sage_tsdf_frustum_bounds(const SageCamera *cam, const float *pose12, double max_depth, double bounds[6]);
int  sage_tsdf_plan(const double bounds[6], double base_voxel, double max_voxels, double trunc_multiplier, int with_color,
                    SageTsdfPlan *out);
int  sage_tsdf_create(SageWorkspace *ws, const SageTsdfPlan *plan, SageTsdfVolume **out);
void sage_tsdf_destroy(SageTsdfVolume *vol);
int  sage_tsdf_reset(SageTsdfVolume *vol);
int  sage_tsdf_get(SageTsdfVolume *vol, float *tsdf, float *weight, float *color);
int  sage_tsdf_dev(SageTsdfVolume *vol, float **tsdf, float **weight, float **color);
int  sage_tsdf_integrate(SageTsdfVolume *vol, const SageTsdfView *view);
int  sage_tsdf_integrate_batch(SageTsdfVolume *vol, const SageTsdfView *views, int n, int flags);
int  sage_tsdf_integrate_batch_launches(int n);
int  sage_tsdf_view_chunk(void);
int  sage_tsdf_last_stats(SageTsdfVolume *vol, SageTsdfStats *out);
/* The window path.  sage_window_depth_range: the minimum over the positive values and the maximum of the depth maps
 * s (bias + basis code) of the keyframes kfs [n] at the current variables, under the window's video mask (a masked pixel
 * counts as 0; no positive value anywhere: *dmin = 0): what sage_tsdf_frustum_bounds takes as max_depth.  The maps, then one
 * reduction kernel (a workgroup and one writer per keyframe) on the window's stream, finished on the host; drains the stream.
 * Both calls form the listed keyframes' maps in scratch of their own with the kernel of sage_depth_and_grad -- the same bytes
 * that call gives for the same variables; the window's depth batch rounds its dot product differently -- and leave the
 * window's own maps and their bookkeeping alone.
 * sage_window_fuse_tsdf: one sage_tsdf_integrate_batch on the window's stream over the keyframes kfs [n], in the order given,
 * with the depth maps at the current variables (prepared keyframes included), the window's own poses and camera, and
 * cfg.mask_dev as the mask.  std_mode SAGE_TSDF_STD_ONE: the reference's behaviour; SAGE_TSDF_STD_SIGMA: the sigma maps of
 * the stored Sigma as the std image (the zero crossing then lies at the inverse-sigma-weighted mean depth, above), formed in
 * scratch the window owns: SAGE_E_STATE without a current Sigma, SAGE_E_UNSUPPORTED where sage_window_depth_sigma answers it.
 * The volume must live on the window's device (SAGE_E_INVALID otherwise); where its workspace's stream is not the window's
 * the two are ordered with events.  SAGE_E_UNSUPPORTED for a sharded window; SAGE_E_STATE before finalize; SAGE_E_INVALID for
 * NULL, n outside 1 .. SAGE_TSDF_MAX_VIEWS, a bad keyframe or std_mode and what sage_tsdf_integrate_batch refuses. */
int  sage_window_depth_range(SageWindow *w, const int32_t *kfs, int n, float *dmin, float *dmax);
int  sage_window_fuse_tsdf(SageWindow *w, SageTsdfVolume *vol, const int32_t *kfs, int n, int std_mode, float std_floor,
                           float obs_weight, float min_depth);

#ifdef __cplusplus
}
#endif
#endif /* SAGE_BA_H_ */
