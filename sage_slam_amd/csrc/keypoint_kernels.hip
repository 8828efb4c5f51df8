// keypoint_kernels.hip -- the sparse matched-keypoint factors: reprojection (fair loss) and 3-D match geometry
// (fair / L2 / huber / "unbiased"), mapper, loop and tracker variants.
//
// Replaces cuda/reprojection_factor_kernels.cpp of the reference: kernels :27-213 / :215-286 (mapper factor,
// D = 13+CS, [pose0 pose1 code0 scale0]) and :288-366 / :367-415 (tracker, D = 6), hosts :417-628, and
// cuda/match_geometry_factor_kernels.cpp (13 kernels there).
// One description per factor (ReprojFactor<CS, MODE>, MatchGeomFactor<CS, MODE>: D, rows per keypoint, parameter struct,
// row body) and ONE kernel family over it: rows_kernel<F, JAC> / small_kernel<F, JAC>, reduce_kernel, stats_kernel, launched
// by impl<F>.  N is a few hundred keypoints at most (launch-latency, not bandwidth).  Small systems (tracker
// D = 6 / 7, loop closure D = 14): ONE launch -- a single workgroup keeps the weighted rows in LDS and contracts them itself in
// double (r04: tracker frame with a reprojection term 0.28 -> 0.20 ms, with match geometry 0.38 -> 0.23 ms).  The mapper
// factors (D = 13 + CS, 14 + 2 CS), and the small ones past 60 KB of rows: rows written once (the residual is the last
// column) and contracted by D workgroups in double -- two launches per call.  Same conventions as the dense factors:
// world-frame left-perturbation Jacobians, P_pose1 = -P_pose0, weight/num_inliers normalisation, 10*weight fallback without
// inliers.  Then the f4 matching core, and the terms of a window (keypoint_batch_kernel: the same row bodies, every term of
// a window in one launch).
#include <type_traits>

#include "sage_device.h"
#include "sage_internal.h"
#include "keypoint_batch.h"

namespace sage
{

// MODE 0: mapper factor (D = 13+CS), MODE 1: tracker (D = 6)
template <int CS, int MODE>
struct ReprojFactor
{
  using Params = ReprojParams;
  static constexpr int D = reproj_dim(MODE, CS), RPP = kReprojRows;
  static constexpr bool kSmall = D * (D + 1) <= 256; // one thread per entry of [AtA | Atb]: small_kernel can contract it

  // LD: row stride in floats (0: D + 1, the residual column last)
  template <bool JAC, int LD = 0>
  static __device__ __forceinline__ void rows(const Params &p, int idx)
  {
    constexpr int RS = LD ? LD : D + 1;
    const float fx = p.cam.fx, fy = p.cam.fy, cx = p.cam.cx, cy = p.cam.cy;
    const float hm[3] = {p.homo[3 * idx + 0], p.homo[3 * idx + 1], p.homo[3 * idx + 2]};
    float d0;
    int loc = 0;
    if (MODE == 0)
    {
      loc = p.loc[idx];
      float acc = p.bias0[loc]; // reprojection_factor_kernels.cpp:57-64
      for (int i = 0; i < CS; ++i)
        acc += p.basis0[(size_t)loc * CS + i] * p.code0[i];
      d0 = acc * p.scale0;
    }
    else
      d0 = p.dpts0[idx];
    float rh[3], X[3];
  #pragma unroll
    for (int i = 0; i < 3; ++i)
    {
      rh[i] = p.R10[i * 3 + 0] * hm[0] + p.R10[i * 3 + 1] * hm[1] + p.R10[i * 3 + 2] * hm[2];
      X[i] = d0 * rh[i] + p.t10[i];
    }
    const bool pos = X[2] > p.eps; // :74
    const float px = (X[0] / X[2]) * fx + cx, py = (X[1] / X[2]) * fy + cy;
    const float sl = sqrtf(p.loss_param);
    const float diff[2] = {p.matched[2 * idx + 0] - px, p.matched[2 * idx + 1] - py};
    const float nx = fabsf(diff[0]) / sl, ny = fabsf(diff[1]) / sl;
    const float sw[2] = {pos ? sqrtf(1.0f / (p.loss_param * (1.0f + nx))) : 0.f,  // :83-84
                         pos ? sqrtf(1.0f / (p.loss_param * (1.0f + ny))) : 0.f};
    p.serr[idx] = pos ? 2.0f * (nx + ny - logf(1.0f + nx) - logf(1.0f + ny)) : 0.f; // :87-90
    p.sval[idx] = pos ? 1.f : 0.f;
    if (!JAC)
      return;
    const float inv_z = 1.0f / X[2];
    const float x_z = inv_z * X[0], y_z = inv_z * X[1];
    float *row0 = p.rows + ((size_t)idx * 2 + 0) * RS, *row1 = p.rows + ((size_t)idx * 2 + 1) * RS;
    if (MODE == 1)
    {
      const float J0[6] = {fx * inv_z, 0.f, -fx * x_z * inv_z, -fx * x_z * y_z, fx * (1.0f + x_z * x_z), -fx * y_z}; // :348
      const float J1[6] = {0.f, fy * inv_z, -fy * y_z * inv_z, -fy * (1.0f + y_z * y_z), fy * x_z * y_z, fy * x_z};
  #pragma unroll
      for (int j = 0; j < 6; ++j)
      {
        row0[j] = sw[0] * J0[j];
        row1[j] = sw[1] * J1[j];
      }
    }
    else
    {
      const float Jpi[2][3] = {{fx * inv_z, 0.f, -fx * x_z * inv_z}, {0.f, fy * inv_z, -fy * y_z * inv_z}}; // :108-109
      float Xw[3];
  #pragma unroll
      for (int i = 0; i < 3; ++i)
        Xw[i] = d0 * (p.R0[i * 3 + 0] * hm[0] + p.R0[i * 3 + 1] * hm[1] + p.R0[i * 3 + 2] * hm[2]) + p.t0[i];
      Pose p1;
  #pragma unroll
      for (int i = 0; i < 9; ++i)
        p1.R[i] = p.R1[i];
      float dX[3][6];
      dX_dT0(p1, Xw, dX); // R1^T [I | -[Xw]x]  (:148-161); dX/dT1 = -dX/dT0 (:124-133)
  #pragma unroll
      for (int j = 0; j < 6; ++j)
      {
        const float a0 = Jpi[0][0] * dX[0][j] + Jpi[0][1] * dX[1][j] + Jpi[0][2] * dX[2][j];
        const float a1 = Jpi[1][0] * dX[0][j] + Jpi[1][1] * dX[1][j] + Jpi[1][2] * dX[2][j];
        row0[j] = sw[0] * a0;
        row1[j] = sw[1] * a1;
        row0[6 + j] = sw[0] * (-a0);
        row1[6 + j] = sw[1] * (-a1);
      }
      const float jd0 = fx * (rh[0] * inv_z - X[0] * rh[2] * inv_z * inv_z); // :175-176
      const float jd1 = fy * (rh[1] * inv_z - X[1] * rh[2] * inv_z * inv_z);
      for (int i = 0; i < CS; ++i)
      {
        const float b = p.basis0[(size_t)loc * CS + i];
        row0[12 + i] = sw[0] * (jd0 * p.scale0 * b); // :182-183
        row1[12 + i] = sw[1] * (jd1 * p.scale0 * b);
      }
      row0[12 + CS] = sw[0] * (jd0 * d0 / p.scale0); // :186
      row1[12 + CS] = sw[1] * (jd1 * d0 / p.scale0);
    }
    row0[D] = sw[0] * diff[0]; // :188-189
    row1[D] = sw[1] * diff[1];
  }
};

// ------------------------------------------------------------------------------------------------
// match geometry: 3 residuals per matched keypoint, W (X1_matched - X0_in_1)
//   MODE 0 mapper  D = 14+2CS [pose0 pose1 code0 code1 scale0 scale1]  (match_geometry_factor_kernels.cpp:421-1041)
//   MODE 1 loop    D = 14     [pose0 pose1 scale0 scale1], unscaled depths handed over          (:296-419)
//   MODE 2 tracker D = 6      relative pose                                                      (:136-213)
//   MODE 3 tracker D = 7      relative pose + scale0                                             (:215-294)
//   loss 0 fair, 1 L2, 2 huber, 3 unbiased (mapper only)
// Normalisation: weight * mean over the N keypoints (hosts :1352-1858); every keypoint counts (sval = 1).
// ------------------------------------------------------------------------------------------------
template <int CS, int MODE>
struct MatchGeomFactor
{
  using Params = MgParams;
  static constexpr int D = mg_dim(MODE, CS), RPP = kMgRows;
  static constexpr bool kSmall = D * (D + 1) <= 256;

  // FINE: the fair loss's error as n - log1p(n).  In fp32 `1 + n` rounds by 6e-8, which is all there is of n - log(1 + n)
  // once n < 3e-4: an LM iteration on terms whose residuals vanish at the solution (a pose graph over exact depths) then
  // compares rounding noise and stops 1e-5 short of it.  The window's loop-MG terms ask for it; the per-edge operators keep
  // the reference's expression
  template <bool JAC, int LD = 0, bool FINE = false>
  static __device__ __forceinline__ void rows(const Params &p, int idx)
  {
    constexpr int RS = LD ? LD : D + 1;
    const float h0[3] = {p.homo0[3 * idx + 0], p.homo0[3 * idx + 1], p.homo0[3 * idx + 2]};
    const float h1[3] = {p.homo1[3 * idx + 0], p.homo1[3 * idx + 1], p.homo1[3 * idx + 2]};
    const float ss = p.scale0 + p.scale1;
    float d0, d1;
    int l0 = 0, l1 = 0;
    if (MODE == 0)
    {
      l0 = p.loc0[idx];
      l1 = p.loc1[idx];
      float a0 = p.bias0[l0], a1 = p.bias1[l1]; // :601-616
      for (int i = 0; i < CS; ++i)
        a0 += p.basis0[(size_t)l0 * CS + i] * p.code0[i];
      for (int i = 0; i < CS; ++i)
        a1 += p.basis1[(size_t)l1 * CS + i] * p.code1[i];
      if (p.loss == 3) // :429-447
      {
        d0 = a0 * p.scale0 / ss;
        d1 = a1 * p.scale1 / ss;
      }
      else
      {
        d0 = a0 * p.scale0;
        d1 = a1 * p.scale1;
      }
    }
    else if (MODE == 1)
    {
      d0 = p.dpts0[idx] * p.scale0; // :303-304
      d1 = p.dpts1[idx] * p.scale1;
    }
    else
    {
      d0 = p.dpts0[idx];
      d1 = p.dpts1[idx];
    }
    float rh[3], X[3], diff[3], sw[3];
  #pragma unroll
    for (int i = 0; i < 3; ++i)
    {
      rh[i] = p.R10[i * 3 + 0] * h0[0] + p.R10[i * 3 + 1] * h0[1] + p.R10[i * 3 + 2] * h0[2];
      X[i] = d0 * rh[i] + p.t10[i];
      diff[i] = d1 * h1[i] - X[i];
    }
    float err = 0.f;
    if (p.loss == 1) // L2 (:792-797)
    {
      sw[0] = sw[1] = sw[2] = 1.f;
      err = diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2];
    }
    else if (p.loss == 2) // huber (:935-962)
    {
  #pragma unroll
      for (int i = 0; i < 3; ++i)
      {
        const float sq = diff[i] * diff[i];
        err += (sq <= p.loss_param) ? sq : (2.0f * sqrtf(p.loss_param * sq) - p.loss_param);
        sw[i] = fminf(1.0f, sqrtf(p.loss_param / sq));
      }
    }
    else // fair (:640-656), also the "unbiased" variant
    {
      const float sl = sqrtf(p.loss_param);
  #pragma unroll
      for (int i = 0; i < 3; ++i)
      {
        const float n = fabsf(diff[i]) / sl;
        err += FINE ? n - log1pf(n) : n - logf(1.0f + n);
        sw[i] = sqrtf(1.0f / (p.loss_param * (1.0f + n)));
      }
      err *= 2.0f;
    }
    p.serr[idx] = err;
    p.sval[idx] = 1.f;
    if (!JAC)
      return;
    float dX[3][6];
    if (MODE <= 1)
    {
      float Xw[3];
  #pragma unroll
      for (int i = 0; i < 3; ++i)
        Xw[i] = d0 * (p.R0[i * 3 + 0] * h0[0] + p.R0[i * 3 + 1] * h0[1] + p.R0[i * 3 + 2] * h0[2]) + p.t0[i];
      Pose p1;
  #pragma unroll
      for (int i = 0; i < 9; ++i)
        p1.R[i] = p.R1[i];
      dX_dT0(p1, Xw, dX); // R1^T [I | -[Xw]x] (:694-705); pose 1 gets the negative (:673-683)
    }
    else
    {
      const float E[3][6] = {{1, 0, 0, 0, X[2], -X[1]}, {0, 1, 0, -X[2], 0, X[0]}, {0, 0, 1, X[1], -X[0], 0}}; // :197-199
  #pragma unroll
      for (int i = 0; i < 3; ++i)
  #pragma unroll
        for (int j = 0; j < 6; ++j)
          dX[i][j] = E[i][j];
    }
  #pragma unroll
    for (int i = 0; i < 3; ++i)
    {
      float *row = p.rows + ((size_t)idx * 3 + i) * RS;
  #pragma unroll
      for (int j = 0; j < 6; ++j)
      {
        row[j] = sw[i] * dX[i][j];
        if (MODE <= 1)
          row[6 + j] = sw[i] * (-dX[i][j]);
      }
      if (MODE == 0)
      {
        const float *b0 = p.basis0 + (size_t)l0 * CS, *b1 = p.basis1 + (size_t)l1 * CS;
        if (p.loss == 3)
        {
          for (int j = 0; j < CS; ++j)
          {
            row[12 + j] = sw[i] * (rh[i] * b0[j] * p.scale0 / ss); // :560-563
            row[12 + CS + j] = sw[i] * (-h1[i] * b1[j] * p.scale1 / ss);
          }
          row[12 + 2 * CS] = sw[i] * (rh[i] * d0 * p.scale1 / (p.scale0 * ss) + h1[i] * d1 / ss); // :566-569
          row[13 + 2 * CS] = sw[i] * (-rh[i] * d0 / ss - h1[i] * d1 * p.scale0 / (p.scale1 * ss));
        }
        else
        {
          for (int j = 0; j < CS; ++j)
          {
            row[12 + j] = sw[i] * (rh[i] * p.scale0 * b0[j]); // :716-719
            row[12 + CS + j] = sw[i] * (-h1[i] * p.scale1 * b1[j]);
          }
          row[12 + 2 * CS] = sw[i] * (rh[i] * d0 / p.scale0); // :722-723
          row[13 + 2 * CS] = sw[i] * (-h1[i] * d1 / p.scale1);
        }
      }
      else if (MODE == 1)
      {
        row[12] = sw[i] * (rh[i] * p.dpts0[idx]); // :398-399
        row[13] = sw[i] * (-h1[i] * p.dpts1[idx]);
      }
      else if (MODE == 3)
        row[6] = sw[i] * (rh[i] * p.dpts0[idx] / p.scale0); // :278
      row[D] = sw[i] * diff[i];
    }
  }
};

// ---- {inliers, error} over the N keypoints in double: each thread its strided sum, then a 256-slot tree (all 256 threads)
struct KpSums
{
  double n, e;
};

__device__ __forceinline__ KpSums kp_sums(const float *serr, const float *sval, int N)
{
  __shared__ double s_n[256], s_e[256];
  const int tid = threadIdx.x;
  double n_in = 0.0, se = 0.0;
  for (int i = tid; i < N; i += 256)
  {
    n_in += (double)sval[i];
    se += (double)serr[i];
  }
  s_n[tid] = n_in;
  s_e[tid] = se;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1)
  {
    if (tid < off)
    {
      s_n[tid] += s_n[tid + off];
      s_e[tid] += s_e[tid + off];
    }
    __syncthreads();
  }
  return {s_n[0], s_e[0]};
}

__device__ __forceinline__ double kp_scale(float weight, const KpSums &s) { return s.n > 0.0 ? (double)weight / s.n : 0.0; }

// stats = {error, num_inliers}: weight * mean, 10 * weight without inliers (:457-464, :507, :523).  The linearize passes
// scale the error like AtA / Atb (by weight / n), the error-only passes divide last
template <bool JAC>
__device__ __forceinline__ void kp_store_stats(float *stats, float weight, const KpSums &s)
{
  if (JAC)
    stats[0] = s.n > 0.0 ? (float)(kp_scale(weight, s) * s.e) : weight * 10.0f;
  else
    stats[0] = s.n > 0.0 ? (float)((double)weight * s.e / s.n) : weight * 10.0f;
  stats[1] = (float)s.n;
}

template <class F, bool JAC>
__global__ __launch_bounds__(256) void rows_kernel(const typename F::Params p)
{
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < p.N)
    F::template rows<JAC>(p, idx);
}

// ---- one launch for the small systems (r04; tracker D = 6 / 7, loop closure D = 14): ONE workgroup writes the weighted
// rows of all keypoints into LDS and contracts them itself -- entry (a, j) of [AtA | Atb] by 256 / (D (D + 1)) threads over
// interleaved rows in double, folded in a fixed order -- instead of rows to memory + a D-workgroup reduce launch.  A tracker
// evaluation is launch-latency bound: one launch less per keypoint term and evaluation.
//   dynamic LDS: the working set of kp_place, then the partial sums
// (the body: small_kernel runs it for the one factor of its arguments, small_batch_kernel for the problem of its workgroup)
template <class F, bool JAC>
__device__ __forceinline__ void small_body(typename F::Params &p, const KpOut &out, float *s_dyn)
{
  constexpr int D = F::D;
  constexpr int NENT = D * (D + 1); // (a, j): a < D, j <= D (j == D: the residual column -> Atb)
  constexpr int NGRP = 256 / NENT;  // row groups (D = 6: 6, D = 7: 4, D = 14: 1)
  static_assert(F::kSmall && NGRP >= 1, "system too large for the one-workgroup contraction");
  const int tid = threadIdx.x;
  kp_place(p, s_dyn, F::RPP, D);
  for (int idx = tid; idx < p.N; idx += 256)
    F::template rows<JAC>(p, idx);
  __syncthreads();
  if (!JAC)
  {
    const KpSums s = kp_sums(p.serr, p.sval, p.N);
    if (tid == 0)
      kp_store_stats<false>(out.stats, p.weight, s);
    return;
  }
  const size_t nf = kp_rows_floats(F::RPP, p.N, D);
  double *s_part = reinterpret_cast<double *>(s_dyn + nf + (nf & 1)); // (8-byte aligned)
  const int ent = tid % NENT, grp = tid / NENT;
  if (grp < NGRP)
  {
    const int a = ent / (D + 1), j = ent % (D + 1);
    double acc = 0.0;
    for (int k = grp; k < F::RPP * p.N; k += NGRP)
      acc += (double)p.rows[(size_t)k * (D + 1) + a] * (double)p.rows[(size_t)k * (D + 1) + j];
    s_part[grp * NENT + ent] = acc;
  }
  const KpSums s = kp_sums(p.serr, p.sval, p.N);
  const double sc = kp_scale(p.weight, s);
  if (tid < NENT)
  {
    double v = 0.0;
    for (int g = 0; g < NGRP; ++g)
      v += s_part[g * NENT + tid];
    v *= sc;
    const int a = tid / (D + 1), j = tid % (D + 1);
    if (j < D)
      out.AtA[(size_t)a * D + j] = (float)v;
    else
      out.Atb[a] = (float)v;
  }
  if (tid == 0)
    kp_store_stats<true>(out.stats, p.weight, s);
}

template <class F, bool JAC>
__global__ __launch_bounds__(256) void small_kernel(typename F::Params p, const KpOut out)
{
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  small_body<F, JAC>(p, out, s_dyn);
}

// ---- batched tracker (sage_track_frame_batch): the keypoint term of every problem that asked for this kind of evaluation
// in the round, ONE launch, workgroup i = problem requests[i].  small_kernel's contraction on the problem's own rows: the
// same F::rows, the same fold order, the same LDS layout (the launch's dynamic LDS is the largest problem's)
template <class F, bool JAC>
__global__ __launch_bounds__(256) void small_batch_kernel(const KpTrackProblem *probs, const int32_t *requests, const SageCamera cam,
                                                          const float eps)
{
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  const KpTrackProblem &P = probs[requests[blockIdx.x]];
  typename F::Params p{};
  if constexpr (std::is_same<typename F::Params, ReprojParams>::value)
  {
    p.R10 = P.R; p.t10 = P.t; p.dpts0 = P.dpts0; p.homo = P.homo0; p.matched = P.matched_2d;
    p.scale0 = 1.f; p.cam = cam; p.eps = eps; p.loss_param = P.loss_param; p.weight = P.weight; p.N = P.N;
  }
  else
  {
    p.R10 = P.R; p.t10 = P.t; p.homo0 = P.homo0; p.homo1 = P.homo1;
    p.scale0 = JAC ? P.scale0 : 1.f; p.scale1 = 1.f; p.loss_param = P.loss_param; p.weight = P.weight; p.loss = P.loss; p.N = P.N;
    p.dpts0 = P.dpts0; p.dpts1 = P.dpts1;
  }
  small_body<F, JAC>(p, KpOut{P.AtA, P.Atb, P.stats}, s_dyn);
}

hipError_t launch_kp_track_batch(hipStream_t s, int dof, bool jac, const KpTrackProblem *probs, const int32_t *requests,
                                 int n_requests, size_t lds_bytes, const SageCamera &cam, float eps)
{
  if (n_requests < 1 || lds_bytes > kKpSmallLdsMax)
    return hipErrorInvalidValue;
  using R = ReprojFactor<16, 1>;
  using M2 = MatchGeomFactor<16, 2>;
  using M3 = MatchGeomFactor<16, 3>;
  const dim3 g(n_requests), b(256);
  if (dof == 6)
  {
    if (jac)
      hipLaunchKernelGGL((small_batch_kernel<R, true>), g, b, lds_bytes, s, probs, requests, cam, eps);
    else
      hipLaunchKernelGGL((small_batch_kernel<R, false>), g, b, lds_bytes, s, probs, requests, cam, eps);
  }
  else if (dof == 7) // (the tracker's modes: 3 = pose and scale for the linearize, 2 = pose only for the error)
  {
    if (jac)
      hipLaunchKernelGGL((small_batch_kernel<M3, true>), g, b, lds_bytes, s, probs, requests, cam, eps);
    else
      hipLaunchKernelGGL((small_batch_kernel<M2, false>), g, b, lds_bytes, s, probs, requests, cam, eps);
  }
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// workgroup a: AtA[a][:] and Atb[a] = (weight/n) sum_rows J[row][a] * [J[row][:] | r[row]] in double; workgroup 0 also
// writes stats = {error, num_inliers}.  D+1 <= 128 columns x 2 row groups per workgroup (D <= 14+2*32 = 78).
__global__ __launch_bounds__(256) void reduce_kernel(const float *__restrict__ rows, const float *__restrict__ serr,
                                                     const float *__restrict__ sval, int N, int D, float weight,
                                                     float *__restrict__ AtA, float *__restrict__ Atb,
                                                     float *__restrict__ stats, int rows_per_point)
{
  __shared__ double s_acc[2][128];
  const int a = blockIdx.x, tid = threadIdx.x, j = tid & 127, grp = tid >> 7;
  double acc = 0.0;
  if (j <= D)
    for (int k = grp; k < rows_per_point * N; k += 2)
      acc += (double)rows[(size_t)k * (D + 1) + a] * (double)rows[(size_t)k * (D + 1) + j];
  s_acc[grp][j] = acc;
  const KpSums s = kp_sums(serr, sval, N);
  const double sc = kp_scale(weight, s);
  if (tid <= D)
  {
    const double v = sc * (s_acc[0][tid] + s_acc[1][tid]);
    if (tid < D)
      AtA[(size_t)a * D + tid] = (float)v;
    else
      Atb[a] = (float)v;
  }
  if (a == 0 && tid == 0)
    kp_store_stats<true>(stats, weight, s);
}

__global__ __launch_bounds__(256) void stats_kernel(const float *__restrict__ serr, const float *__restrict__ sval, int N,
                                                    float weight, float *__restrict__ stats)
{
  const KpSums s = kp_sums(serr, sval, N);
  if (threadIdx.x == 0)
    kp_store_stats<false>(stats, weight, s);
}

// lays the scratch out once and chooses: one launch where the system is small and its rows fit 60 KB of LDS, else two
template <class F>
static hipError_t impl(hipStream_t s, typename F::Params p, bool jac, float *scratch, const KpOut &out)
{
  constexpr int D = F::D, RPP = F::RPP;
  const int N = p.N, grid = (N + 255) / 256;
  if constexpr (F::kSmall)
  {
    const size_t small_lds = kp_small_lds_bytes(RPP, N, D);
    if (N > 0 && small_lds <= kKpSmallLdsMax)
    {
      if (jac)
        hipLaunchKernelGGL((small_kernel<F, true>), dim3(1), dim3(256), small_lds, s, p, out);
      else
        hipLaunchKernelGGL((small_kernel<F, false>), dim3(1), dim3(256), small_lds, s, p, out);
      return hipGetLastError();
    }
  }
  kp_place(p, scratch, RPP, D);
  if (jac)
  {
    if (grid > 0)
      hipLaunchKernelGGL((rows_kernel<F, true>), dim3(grid), dim3(256), 0, s, p);
    hipLaunchKernelGGL(reduce_kernel, dim3(D), dim3(256), 0, s, p.rows, p.serr, p.sval, N, D, p.weight, out.AtA, out.Atb,
                       out.stats, RPP);
  }
  else
  {
    if (grid > 0)
      hipLaunchKernelGGL((rows_kernel<F, false>), dim3(grid), dim3(256), 0, s, p);
    hipLaunchKernelGGL(stats_kernel, dim3(1), dim3(256), 0, s, p.serr, p.sval, N, p.weight, out.stats);
  }
  return hipGetLastError();
}

hipError_t launch_reproj(hipStream_t s, int CS, bool tracker, bool jac, const ReprojParams &p, float *scratch, const KpOut &out)
{
  if (tracker)
    return impl<ReprojFactor<16, 1>>(s, p, jac, scratch, out);
  if (CS == 32)
    return impl<ReprojFactor<32, 0>>(s, p, jac, scratch, out);
  if (CS == 16)
    return impl<ReprojFactor<16, 0>>(s, p, jac, scratch, out);
  return hipErrorInvalidValue;
}

hipError_t launch_match_geom(hipStream_t s, int mode, int CS, bool jac, const MgParams &p, float *scratch, const KpOut &out)
{
  switch (mode)
  {
  case 0:
    if (CS == 32)
      return impl<MatchGeomFactor<32, 0>>(s, p, jac, scratch, out);
    if (CS == 16)
      return impl<MatchGeomFactor<16, 0>>(s, p, jac, scratch, out);
    return hipErrorInvalidValue;
  case 1:
    return impl<MatchGeomFactor<16, 1>>(s, p, jac, scratch, out);
  case 2:
    return impl<MatchGeomFactor<16, 2>>(s, p, jac, scratch, out);
  case 3:
    return impl<MatchGeomFactor<16, 3>>(s, p, jac, scratch, out);
  default:
    return hipErrorInvalidValue;
  }
}


// ------------------------------------------------------------------------------------------------
// f4 matching core: response-map argmax with cycle consistency (core/gtsam/match_geometry_factor.cpp:62-97,
// core/system/camera_tracker.cpp:608-633).  response[k][p] = -sum_c (q[c][k] - target[c][p])^2 is never materialised
// (the reference builds two K x H*W tensors): one workgroup owns KPB query descriptors (LDS), streams the target
// descriptor map once (coalesced over pixels, channel sum sequential in fp32 like the restated reference) and keeps a
// running (response, index) pair per query and lane; first index wins ties.
// ------------------------------------------------------------------------------------------------
constexpr int kMatchKPB = 8; // queries per workgroup: the target map is read K/8 times instead of K times

__global__ __launch_bounds__(256) void best_match_kernel(const float *__restrict__ query_map, const long long *__restrict__ query_loc,
                                                         const float *__restrict__ target_map, int K, int C, int HW,
                                                         long long *__restrict__ best_out)
{
  extern __shared__ float s_dyn[]; // [KPB][C] query descriptors, then the reduction scratch
  float *s_q = s_dyn;
  const int tid = threadIdx.x, k0 = blockIdx.x * kMatchKPB;
  const int nk = min(kMatchKPB, K - k0);
  for (int i = tid; i < kMatchKPB * C; i += 256)
  {
    const int kk = i / C, c = i - kk * C;
    s_q[i] = kk < nk ? query_map[(size_t)c * HW + query_loc[k0 + kk]] : 0.f;
  }
  __syncthreads();
  float best_r[kMatchKPB];
  int best_p[kMatchKPB];
#pragma unroll
  for (int kk = 0; kk < kMatchKPB; ++kk)
  {
    best_r[kk] = -INFINITY;
    best_p[kk] = 0x7fffffff;
  }
  for (int p = tid; p < HW; p += 256)
  {
    float acc[kMatchKPB];
#pragma unroll
    for (int kk = 0; kk < kMatchKPB; ++kk)
      acc[kk] = 0.f;
    for (int c = 0; c < C; ++c)
    {
      const float t = target_map[(size_t)c * HW + p];
#pragma unroll
      for (int kk = 0; kk < kMatchKPB; ++kk)
      {
        const float d = s_q[kk * C + c] - t;
        acc[kk] = __fadd_rn(acc[kk], __fmul_rn(d, d)); // no FMA contraction: the argmax must not depend on it
      }
    }
#pragma unroll
    for (int kk = 0; kk < kMatchKPB; ++kk)
    {
      const float r = -acc[kk];
      if (r > best_r[kk]) // ascending p per lane: '>' keeps the first maximum
      {
        best_r[kk] = r;
        best_p[kk] = p;
      }
    }
  }
  // cross-lane: larger response wins, equal responses -> smaller index
  float *s_r = s_dyn + kMatchKPB * C;
  int *s_p = reinterpret_cast<int *>(s_r + 256);
  for (int kk = 0; kk < nk; ++kk)
  {
    __syncthreads();
    s_r[tid] = best_r[kk];
    s_p[tid] = best_p[kk];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1)
    {
      if (tid < off)
      {
        const float r2 = s_r[tid + off];
        const int p2 = s_p[tid + off];
        if (r2 > s_r[tid] || (r2 == s_r[tid] && p2 < s_p[tid]))
        {
          s_r[tid] = r2;
          s_p[tid] = p2;
        }
      }
      __syncthreads();
    }
    if (tid == 0)
      best_out[k0 + kk] = s_p[0];
  }
}

__global__ void cycle_flags_kernel(const long long *__restrict__ kp_loc0, const long long *__restrict__ cyc_loc0, int K,
                                   int W, float thresh, int32_t *__restrict__ inlier, int *__restrict__ n_out)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K)
    return;
  const float dx = (float)(kp_loc0[k] % W) - (float)(cyc_loc0[k] % W);
  const float dy = (float)(kp_loc0[k] / W) - (float)(cyc_loc0[k] / W);
  const int in = (dx * dx + dy * dy) <= thresh * thresh; // match_geometry_factor.cpp:91-94
  inlier[k] = in;
  if (in)
    atomicAdd(n_out, 1); // integer count: order independent
}

hipError_t launch_cycle_match(hipStream_t s, const float *desc0, const float *desc1, const long long *kp_loc0, int K,
                              int C, int H, int W, float cyc_thresh, long long *raw_matched1, long long *cyc_matched0,
                              int32_t *inlier, int *n_inliers_dev)
{
  if (K <= 0)
    return hipSuccess;
  const int HW = H * W;
  const size_t shm = ((size_t)kMatchKPB * C + 512) * sizeof(float);
  const int grid = (K + kMatchKPB - 1) / kMatchKPB;
  hipLaunchKernelGGL(best_match_kernel, dim3(grid), dim3(256), shm, s, desc0, kp_loc0, desc1, K, C, HW, raw_matched1);
  hipLaunchKernelGGL(best_match_kernel, dim3(grid), dim3(256), shm, s, desc1, raw_matched1, desc0, K, C, HW, cyc_matched0);
  hipLaunchKernelGGL(cycle_flags_kernel, dim3((K + 255) / 256), dim3(256), 0, s, kp_loc0, cyc_matched0, K, W, cyc_thresh,
                     inlier, n_inliers_dev);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// window terms (sage_window_add_keypoint_term): every local term of a window in ONE launch, a workgroup per term.
// The per-edge operators above write the weighted rows to memory and contract them in a second launch (D workgroups);
// here the rows of kKpChunk keypoints at a time stay in LDS (stride padded to four floats: 64 x 2 x 48 floats = 24 KB for
// reprojection at CS = 32, 64 x 3 x 80 = 60 KB for match geometry, 64 x 3 x 16 = 12 KB for loop-MG) and are contracted into per-thread 4 x 4 register tiles of
// [AtA | Atb] that live across the chunks: two 16-byte LDS reads per 16 multiply-adds.  Only the tiles on and above the
// diagonal are formed (CS = 32: 78 / 210 of them, loop-MG: 10, so 256 / tiles row groups share a chunk's rows -- 3, 1 and
// 25, threads 250-255 idle) and mirrored on the way out.  Sums in double, every order fixed (rows ascending per group, groups ascending, lanes by shuffle): no atomics,
// bit-reproducible.  weight / n_inliers, the 10 * weight fallback and the statistics are folded in by the same workgroup.
// The relative pose is formed here from the window's variable array, as the dense kernels do.
// ------------------------------------------------------------------------------------------------
template <int CS, int KIND, bool JAC>
__device__ __forceinline__ void kp_term_run(const KpTerm &T, const KpBatchParams &prm, const float *s_pose, float *s_rows,
                                            float *s_err, float *s_val, double *s_red)
{
  // KIND 2: the loop variant (MatchGeomFactor mode 1) -- poses and scales from the window, depths from the term
  using F = std::conditional_t<KIND == 0, ReprojFactor<CS, 0>, MatchGeomFactor<CS, KIND == 2 ? 1 : 0>>;
  constexpr int D = F::D, RPP = F::RPP;
  constexpr int LD = (D + 1 + 3) / 4 * 4;
  constexpr int NT = LD / 4;               // tiles per side (rows past D are dropped on the way out)
  constexpr int NTILES = NT * (NT + 1) / 2;
  constexpr int NGRP = 256 / NTILES;
  static_assert(NGRP >= 1, "more tiles than threads");
  static_assert((size_t)NTILES * 16 * sizeof(double) <= (size_t)kKpChunk * RPP * LD * sizeof(float), "group fold scratch");
  const int tid = threadIdx.x;
  const float *x0 = prm.vars + (size_t)T.k0 * prm.VS, *x1 = prm.vars + (size_t)T.k1 * prm.VS;
  ReprojParams rp{};
  MgParams mp{};
  if (KIND == 0)
  {
    rp.R10 = s_pose; rp.t10 = s_pose + 9; rp.R0 = x0; rp.t0 = x0 + 9; rp.R1 = x1; rp.t1 = x1 + 9;
    rp.bias0 = T.bias0; rp.basis0 = T.basis0; rp.code0 = x0 + 13; rp.scale0 = x0[12];
    rp.cam = prm.cam; rp.eps = prm.eps; rp.loss_param = T.loss_param; rp.weight = T.weight;
    rp.rows = s_rows; rp.serr = s_err; rp.sval = s_val;
  }
  else
  {
    mp.R10 = s_pose; mp.t10 = s_pose + 9; mp.R0 = x0; mp.t0 = x0 + 9; mp.R1 = x1; mp.t1 = x1 + 9;
    mp.bias0 = T.bias0; mp.bias1 = T.bias1; mp.basis0 = T.basis0; mp.basis1 = T.basis1;
    mp.code0 = x0 + 13; mp.code1 = x1 + 13; mp.scale0 = x0[12]; mp.scale1 = x1[12];
    mp.loss_param = T.loss_param; mp.weight = T.weight; mp.loss = KIND == 2 ? 0 : T.loss;
    mp.rows = s_rows; mp.serr = s_err; mp.sval = s_val;
  }
  // this thread's tile (ti <= tj) and row group
  const int grp = tid / NTILES;
  const bool active = JAC && grp < NGRP;
  int ti = 0, tj = 0;
  {
    int rem = tid % NTILES;
    while (rem >= NT - ti)
    {
      rem -= NT - ti;
      ++ti;
    }
    tj = ti + rem;
  }
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = 0.0;
  double se = 0.0, sn = 0.0; // lanes of wave 0: keypoint `lane` of every chunk
  for (int c0 = 0; c0 < T.N; c0 += kKpChunk)
  {
    const int cnt = min(kKpChunk, T.N - c0);
    if (tid < cnt)
    {
      if (KIND == 0)
      {
        rp.loc = T.loc0 + c0; rp.homo = T.homo0 + (size_t)3 * c0; rp.matched = T.matched + (size_t)2 * c0; rp.N = cnt;
        ReprojFactor<CS, 0>::template rows<JAC, LD>(rp, tid);
      }
      else
      {
        if (KIND == 2)
        {
          mp.dpts0 = T.dpts0 + c0; mp.dpts1 = T.dpts1 + c0;
        }
        else
        {
          mp.loc0 = T.loc0 + c0; mp.loc1 = T.loc1 + c0;
        }
        mp.homo0 = T.homo0 + (size_t)3 * c0; mp.homo1 = T.homo1 + (size_t)3 * c0;
        mp.N = cnt;
        MatchGeomFactor<CS, KIND == 2 ? 1 : 0>::template rows<JAC, LD, KIND == 2>(mp, tid);
      }
      if (JAC)
        for (int r = 0; r < RPP; ++r) // the padding columns take part in the tiles: keep them finite
          for (int c = D + 1; c < LD; ++c)
            s_rows[((size_t)tid * RPP + r) * LD + c] = 0.f;
    }
    __syncthreads();
    if (tid < cnt)
    {
      se += (double)s_err[tid];
      sn += (double)s_val[tid];
    }
    if (active)
    {
      const float *ra = s_rows + 4 * ti, *rb = s_rows + 4 * tj;
      for (int k = grp; k < RPP * cnt; k += NGRP)
      {
        const float4 a = *reinterpret_cast<const float4 *>(ra + (size_t)k * LD);
        const float4 b = *reinterpret_cast<const float4 *>(rb + (size_t)k * LD);
        const double av[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
        const double bv[4] = {(double)b.x, (double)b.y, (double)b.z, (double)b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] += av[i] * bv[j];
      }
    }
    __syncthreads();
  }
  // statistics: wave 0, fixed lane order
  if (tid < 64)
  {
    for (int off = 32; off > 0; off >>= 1)
    {
      se += __shfl_down(se, off);
      sn += __shfl_down(sn, off);
    }
    if (tid == 0)
    {
      s_red[0] = sn;
      s_red[1] = se;
    }
  }
  __syncthreads();
  const double ninl = s_red[0];
  const double sc = ninl > 0.0 ? (double)T.weight / ninl : 0.0;
  if (tid == 0)
  {
    prm.out.stats[2 * (size_t)T.stat + 0] = ninl > 0.0 ? (float)(sc * s_red[1]) : T.weight * 10.0f;
    prm.out.stats[2 * (size_t)T.stat + 1] = (float)ninl;
  }
  if (!JAC)
    return;
  // row groups folded into group 0, one after the other (the rows' LDS is free now)
  double *s_fold = reinterpret_cast<double *>(s_rows);
  for (int g = 1; g < NGRP; ++g)
  {
    if (grp == g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          s_fold[((size_t)(i * 4 + j)) * NTILES + tid % NTILES] = acc[i][j];
    __syncthreads();
    if (grp == 0)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] += s_fold[((size_t)(i * 4 + j)) * NTILES + tid];
    __syncthreads();
  }
  if (grp != 0)
    return;
  constexpr int G = plan::keypoint_kind_group(KIND);
  static_assert(TermResults::dim(G, CS) == D, "the kind's group");
  float *AtA = prm.out.AtA(G) + (size_t)T.out * D * D;
  float *Atb = prm.out.Atb(G) + (size_t)T.out * D;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
    {
      const int r = 4 * ti + i, c = 4 * tj + j;
      if (r >= D || c > D)
        continue;
      const float v = (float)(sc * acc[i][j]);
      if (c == D)
        Atb[r] = v;
      else
      {
        AtA[(size_t)r * D + c] = v;
        if (ti != tj)
          AtA[(size_t)c * D + r] = v;
      }
    }
}

template <int CS, bool JAC>
__global__ __launch_bounds__(256) void keypoint_batch_kernel(const KpBatchParams prm)
{
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  __shared__ float s_pose[12], s_err[kKpChunk], s_val[kKpChunk];
  __shared__ double s_red[2];
  const KpTerm T = prm.terms[blockIdx.x];
  if (threadIdx.x == 0)
  {
    const Pose p10 = relative_pose(load_pose(prm.vars + (size_t)T.k0 * prm.VS), load_pose(prm.vars + (size_t)T.k1 * prm.VS));
#pragma unroll
    for (int i = 0; i < 9; ++i)
      s_pose[i] = p10.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      s_pose[9 + i] = p10.t[i];
  }
  __syncthreads();
  if (T.kind == SAGE_KP_REPROJECTION)
    kp_term_run<CS, 0, JAC>(T, prm, s_pose, s_dyn, s_err, s_val, s_red);
  else if (T.kind == SAGE_KP_MATCH_GEOMETRY)
    kp_term_run<CS, 1, JAC>(T, prm, s_pose, s_dyn, s_err, s_val, s_red);
  else
    kp_term_run<CS, 2, JAC>(T, prm, s_pose, s_dyn, s_err, s_val, s_red);
}

hipError_t launch_keypoint_batch(hipStream_t s, int CS, bool jac, int n_terms, unsigned kinds, const KpBatchParams &p)
{
  if (n_terms <= 0)
    return hipSuccess;
  const size_t lds = jac ? kp_batch_lds_bytes(CS, kinds) : 0; // (the error variant forms no rows)
  if (CS == 32)
  {
    if (jac)
      hipLaunchKernelGGL((keypoint_batch_kernel<32, true>), dim3(n_terms), dim3(256), lds, s, p);
    else
      hipLaunchKernelGGL((keypoint_batch_kernel<32, false>), dim3(n_terms), dim3(256), lds, s, p);
  }
  else if (CS == 16)
  {
    if (jac)
      hipLaunchKernelGGL((keypoint_batch_kernel<16, true>), dim3(n_terms), dim3(256), lds, s, p);
    else
      hipLaunchKernelGGL((keypoint_batch_kernel<16, false>), dim3(n_terms), dim3(256), lds, s, p);
  }
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

} // namespace sage
