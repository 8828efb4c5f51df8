// keypoint_batch.h -- the matched-keypoint terms of a window (sage_window_add_keypoint_term): device table row and the
// launch of the batched kernel (keypoint_kernels.hip), shared with the window engine (window.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sage_ba.h"

namespace sage
{

constexpr int kKpChunk = 64; // keypoints whose weighted rows sit in LDS at a time

// one term = one workgroup.  kind 0 reprojection (D = 13+CS, the photometric edge layout), 1 match geometry (D = 14+2CS,
// the geometric edge layout).  All arrays engine-owned (copied at add / finalize), keyframe data the window's own.
struct KpTerm
{
  int32_t kind, loss, N;
  int32_t out;    // index among the local terms of its kind: where AtA / Atb go
  int32_t stat;   // index among all local terms (reprojection first): where {error, inliers} go
  int32_t k0, k1; // keyframes "0" and "1" of the directed edge
  float loss_param, weight;
  const int32_t *loc0, *loc1;           // [N]; loc1: match geometry
  const float *homo0, *homo1, *matched; // [N,3], [N,3] (match geometry), [N,2] (reprojection)
  const float *bias0, *basis0, *bias1, *basis1;
};

struct KpBatchParams
{
  const KpTerm *terms;
  const float *vars; // [K][VS]: pose 12, scale, code CS -- the variable set being evaluated
  int VS;
  SageCamera cam;
  float eps;
  float *AtA_r, *Atb_r, *AtA_m, *Atb_m; // per kind [n][D*D], [n][D] (linearize only)
  float *stats;                         // [n_terms][2] = {error, inliers}
};

// dynamic LDS of the batched kernel: the chunk's rows, stride padded to four floats
inline size_t kp_batch_lds_bytes(int CS, bool any_match_geometry)
{
  const int D = any_match_geometry ? 14 + 2 * CS : 13 + CS, rpp = any_match_geometry ? 3 : 2;
  return (size_t)kKpChunk * rpp * (size_t)((D + 1 + 3) / 4 * 4) * sizeof(float);
}

// every local term of a window in ONE launch (a workgroup per term); jac = false: errors and inlier counts only
hipError_t launch_keypoint_batch(hipStream_t s, int CS, bool jac, int n_terms, bool any_match_geometry,
                                 const KpBatchParams &p);

} // namespace sage
