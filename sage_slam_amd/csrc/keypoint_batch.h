// keypoint_batch.h -- what the host units see of the matched-keypoint factors (keypoint_kernels.hip): system sizes and
// scratch layout, the parameter / output structs and launches of the per-edge operators (operators.hip), and the device
// table row and launch of a window's terms (sage_window_add_keypoint_term; window_eval.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sage_ba.h"
#include "term_results.h"

namespace sage
{

// system size D by factor, mode and code size; rows per keypoint
//   reprojection    mode 0 mapper [pose0 pose1 code0 scale0], 1 tracker (relative pose)
//   match geometry  mode 0 mapper [pose0 pose1 code0 code1 scale0 scale1], 1 loop [pose0 pose1 scale0 scale1],
//                   2 tracker (relative pose), 3 tracker (relative pose + scale0)
constexpr int reproj_dim(int mode, int CS) { return mode == 0 ? 13 + CS : 6; }
constexpr int mg_dim(int mode, int CS) { return mode == 0 ? 14 + 2 * CS : (mode == 1 ? 14 : (mode == 2 ? 6 : 7)); }
constexpr int kReprojRows = 2, kMgRows = 3;

// one factor evaluation's working set: weighted rows [rpp * N][D + 1] (the residual is the last column) | serr [N] | sval [N]
constexpr size_t kp_rows_floats(int rpp, int N, int D) { return (size_t)rpp * N * (D + 1) + (size_t)2 * N; }
constexpr size_t kp_scratch_floats(int rpp, int N, int D) { return kp_rows_floats(rpp, N, D) + 4; }
template <class P>
__host__ __device__ inline void kp_place(P &p, float *base, int rpp, int D)
{
  p.rows = base;
  p.serr = base + (size_t)rpp * p.N * (D + 1);
  p.sval = p.serr + p.N;
}

struct ReprojParams
{
  const float *R10, *t10, *R0, *t0, *R1, *t1; // mapper: all six; tracker: R10/t10 = the relative pose
  const float *bias0, *basis0, *code0;        // mapper
  const int32_t *loc;                         // mapper
  const float *dpts0;                         // tracker: sampled depths [N]
  const float *homo, *matched;                // [N,3], [N,2]
  float scale0;
  SageCamera cam;
  float eps, loss_param, weight;
  int N;
  float *rows, *serr, *sval; // placed by the launch (kp_place)
};

// loss 0 fair, 1 L2, 2 huber, 3 unbiased (mapper only)
struct MgParams
{
  const float *R10, *t10, *R0, *t0, *R1, *t1;
  const float *bias0, *bias1, *basis0, *basis1, *code0, *code1; // mode 0
  const float *dpts0, *dpts1;                                   // mode 1: unscaled; mode 2/3: scaled
  const float *homo0, *homo1;
  const int32_t *loc0, *loc1;
  float scale0, scale1, loss_param, weight;
  int loss, N;
  float *rows, *serr, *sval;
};

struct KpOut
{
  float *AtA, *Atb; // [D][D], [D]: jac only
  float *stats;     // {error, num_inliers}
};

// the one-workgroup contraction (small_kernel): its dynamic LDS -- the working set, then 256 partial sums in double -- and
// what a workgroup may ask for
constexpr size_t kKpSmallLdsMax = 60 * 1024;
constexpr size_t kp_small_lds_bytes(int rpp, int N, int D) { return (kp_rows_floats(rpp, N, D) + 2) * sizeof(float) + (size_t)256 * sizeof(double); }
// (N = 512 matches at D = 7: (3 * 512 * 8 + 1024 + 2) * 4 + 2048 = 55 304 bytes -- the loop detector's NK <= 512 stays on the
// one-launch path, in sage_track_frame and in a batch alike)

// one problem of a batched tracker call (sage_track_frame_batch), in the call's pinned table: written once per call, scale0
// before every round the problem takes part in
struct KpTrackProblem
{
  const float *R, *t;        // the pose slot of the problem's TrackHost
  const float *dpts0, *homo0; // [N], [N,3]: the caller's metric depths (dof 6) or the problem's slice of the round's scaled ones
  const float *matched_2d;   // dof 6: [N,2]
  const float *dpts1, *homo1; // dof 7: [N], [N,3]
  float scale0;              // per round: the scale being evaluated
  float loss_param, weight;
  int32_t N, loss;           // loss: SAGE_LOSS_FAIR -- read from the table like every other parameter, so that the rows'
                             // code is compiled as in small_kernel (a constant here would prune and re-fuse it)
  float *AtA, *Atb, *stats;  // the keypoint slots of the problem's TrackHost
};
// dof 6: reprojection, dof 7: match geometry (mode 3 with jac, mode 2 without, as sage_track_frame evaluates them); a
// workgroup per request; lds_bytes: the largest kp_small_lds_bytes among them
hipError_t launch_kp_track_batch(hipStream_t s, int dof, bool jac, const KpTrackProblem *probs, const int32_t *requests,
                                 int n_requests, size_t lds_bytes, const SageCamera &cam, float eps);

// scratch: kp_scratch_floats(rows per keypoint, N, D) floats
hipError_t launch_reproj(hipStream_t s, int CS, bool tracker, bool jac, const ReprojParams &p, float *scratch, const KpOut &out);
hipError_t launch_match_geom(hipStream_t s, int mode, int CS, bool jac, const MgParams &p, float *scratch, const KpOut &out);

constexpr int kKpChunk = 64; // keypoints whose weighted rows sit in LDS at a time

// one term = one workgroup.  kind 0 reprojection (D = 13+CS, the photometric edge layout), 1 match geometry (D = 14+2CS,
// the geometric edge layout), 2 loop-MG (D = 14: match geometry at fixed depths, poses and scales only).  All arrays
// engine-owned (copied at add / finalize), keyframe data the window's own.
struct KpTerm
{
  int32_t kind, loss, N;
  int32_t out;    // where AtA / Atb go in the kind's group, where {error, inliers} go: plan::term_layout
  int32_t stat;
  int32_t k0, k1; // keyframes "0" and "1" of the directed edge
  float loss_param, weight;
  const int32_t *loc0, *loc1;           // [N]; loc1: match geometry
  const float *homo0, *homo1, *matched; // [N,3], [N,3] (match geometry), [N,2] (reprojection)
  const float *bias0, *basis0, *bias1, *basis1;
  const float *dpts0, *dpts1; // [N] each, unscaled (loop-MG)
};

struct KpBatchParams
{
  const KpTerm *terms;
  const float *vars; // [K][VS]: pose 12, scale, code CS -- the variable set being evaluated
  int VS;
  SageCamera cam;
  float eps;
  TermResults out;   // AtA / Atb: linearize only
};

// system size and rows per keypoint of a window term by kind (SAGE_KP_*)
constexpr int kp_kind_dim(int kind, int CS) { return kind == 0 ? reproj_dim(0, CS) : (kind == 1 ? mg_dim(0, CS) : mg_dim(1, CS)); }
constexpr int kp_kind_rows(int kind) { return kind == 0 ? kReprojRows : kMgRows; }
constexpr int kKpKinds = plan::kKeypointKinds;

// dynamic LDS of the batched kernel: a chunk's rows, stride padded to four floats -- the largest over the kinds PRESENT
// among the launch's terms (kinds: bit k = a term of kind k; CS = 32: 24 KB, 60 KB, 12 KB)
inline size_t kp_batch_lds_bytes(int CS, unsigned kinds)
{
  size_t bytes = 0;
  for (int kind = 0; kind < kKpKinds; ++kind)
    if (kinds & (1u << kind))
      bytes = std::max(bytes, (size_t)kKpChunk * kp_kind_rows(kind) * (size_t)((kp_kind_dim(kind, CS) + 1 + 3) / 4 * 4) * sizeof(float));
  return bytes;
}

// every local term of a window in ONE launch (a workgroup per term); jac = false: errors and inlier counts only
hipError_t launch_keypoint_batch(hipStream_t s, int CS, bool jac, int n_terms, unsigned kinds, const KpBatchParams &p);

} // namespace sage
