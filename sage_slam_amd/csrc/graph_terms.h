// graph_terms.h -- the pose-graph terms of a window (sage_window_add_graph_term): the factors of the reference's live
// loop-closure graph, DeepFactors::LoopClosurePoseScaleEstimate (core/deepfactors.cpp:58-386) --
//   graph_rel_pose_scale   RelPoseScaleFactor  (core/gtsam/rel_pose_scale_factor.cpp:207-344)   7 residuals
//   graph_rel_pose         RelPoseFactor       (core/gtsam/rel_pose_factor.cpp:150-262)         6 residuals
//   graph_scale_prior      ScaleFactor         (core/gtsam/scale_factor.cpp:102-129)            1 residual
// each written once for the device kernel (graph_kernels.hip) and for a host compiler (tests/test_window_graph_terms_api.py
// compiles this header on its own).  Plain C++17, fp32, no HIP include: SAGE_HD as in damped_system.h.
//
// Every kind fills the same J [7][14] (columns [pose0(6) pose1(6) scale0 scale1], tangent [translation, rotation] of the
// window's LEFT retraction T <- exp(delta) T; rows and columns a kind does not have are zero) and r [7] = target - current,
// and returns error = weight * |r|^2; the caller forms AtA = weight * J^T J, Atb = weight * J^T r.
//
// The error is the reference's as written.  The Jacobian is its exact derivative, which is NOT the reference's matrix in two
// places: (1) rel_pose_scale_factor.cpp:288 / rel_pose_factor.cpp:229 build d pose10 / d pose1^-1 as kron(pose0, I3) where
// the derivative is kron(pose0^T, I3) -- with the transpose the pose1 block is exactly minus the pose0 block, the closed form
// used here; (2) rel_pose_scale_factor.cpp:320 puts -target_t / s0^2 into the translation rows of the scale0 column where the
// derivative of t10 / s0 is -t10 / s0^2.  log R and its derivative do not copy the reference's fp32 sin = sqrt(1 - cos^2) or
// its exact-equality small-angle switch: atan2 of (|axis part|, cos) with series below sin^2 = 1e-2, accurate from the identity
// (log = 0 exactly) to theta = 2.5; theta near pi is outside the reference's formula and outside this one.
#pragma once
#include <cmath>
#include <cstdint>

#include "damped_system.h" // SAGE_HD

namespace sage
{

constexpr int kGraphD = 14, kGraphRows = 7;
enum : int { kGraphRelPoseScale = 0, kGraphRelPose = 1, kGraphScalePrior = 2 }; // = SAGE_GRAPH_*

// residuals per term by kind
constexpr int graph_kind_rows(int kind) { return kind == kGraphRelPoseScale ? 7 : (kind == kGraphRelPose ? 6 : 1); }

// one term as the kernel reads it (the device table's row)
struct GraphTerm
{
  int32_t kind;
  int32_t k0, k1; // keyframes "0" and "1" of the directed edge; a scale prior: k0 = k1 = its keyframe
  int32_t out;    // where AtA / Atb go in the pose-scale group, where {error, residuals} go: plan::term_layout
  int32_t stat;
  float target[12]; // of pose1^-1 * pose0: R row-major, then t
  float ts0, ts1;   // target scales; a scale prior uses ts0
  float weight, rot_weight, scale_weight;
};

// log of a rotation matrix (row-major) and theta^2 = |phi|^2
SAGE_HD inline void so3_log(const float *R, float phi[3], float &theta2)
{
  const float a[3] = {0.5f * (R[7] - R[5]), 0.5f * (R[2] - R[6]), 0.5f * (R[3] - R[1])}; // sin(theta) * axis
  const float s2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  const float c = 0.5f * (R[0] + R[4] + R[8] - 1.0f);
  float k; // theta / sin(theta)
  if (c > 0.f && s2 < 1.0e-2f)
    k = 1.0f + s2 * (1.0f / 6.0f + s2 * (3.0f / 40.0f + s2 * (5.0f / 112.0f + s2 * (35.0f / 1152.0f)))); // asin(s) / s
  else
  {
    const float s = sqrtf(s2);
    k = atan2f(s, c) / s;
  }
  phi[0] = k * a[0];
  phi[1] = k * a[1];
  phi[2] = k * a[2];
  theta2 = k * k * s2;
}

// inverse of the left Jacobian of SO(3): log(exp(e) R) = phi + Jl^-1(phi) e + O(e^2)
//   Jl^-1 = I - [phi]x / 2 + c (phi phi^T - theta^2 I),   c = (1 - (theta / 2) cot(theta / 2)) / theta^2
SAGE_HD inline void so3_left_jacobian_inverse(const float phi[3], float theta2, float Ji[3][3])
{
  float c;
  if (theta2 < 1.0e-2f)
    c = 1.0f / 12.0f + theta2 * (1.0f / 720.0f + theta2 * (1.0f / 30240.0f));
  else
  {
    const float h = 0.5f * sqrtf(theta2);
    c = (1.0f - h * cosf(h) / sinf(h)) / theta2;
  }
  const float hx[3][3] = {{0.f, -phi[2], phi[1]}, {phi[2], 0.f, -phi[0]}, {-phi[1], phi[0], 0.f}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      Ji[i][j] = (i == j ? 1.0f - c * theta2 : 0.f) - 0.5f * hx[i][j] + c * phi[i] * phi[j];
}

// the two binary kinds.  SCALE: translation over scale0, the log-scale-ratio row and the two scale columns
template <bool SCALE, bool JAC>
SAGE_HD inline float graph_rel_pose_body(const float *pose0, const float *pose1, float s0, float s1, const GraphTerm &t,
                                         float J[kGraphRows][kGraphD], float r[kGraphRows])
{
  const float *R0 = pose0, *t0 = pose0 + 9, *R1 = pose1, *t1 = pose1 + 9;
  float R10[9], t10[3];
  const float d[3] = {t0[0] - t1[0], t0[1] - t1[1], t0[2] - t1[2]};
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j)
      R10[i * 3 + j] = R1[0 * 3 + i] * R0[0 * 3 + j] + R1[1 * 3 + i] * R0[1 * 3 + j] + R1[2 * 3 + i] * R0[2 * 3 + j];
    t10[i] = R1[0 * 3 + i] * d[0] + R1[1 * 3 + i] * d[1] + R1[2 * 3 + i] * d[2];
  }
  float phi[3], th2, phit[3], th2t;
  so3_log(R10, phi, th2);
  so3_log(t.target, phit, th2t);
  const float inv_s0 = SCALE ? 1.0f / s0 : 1.0f, inv_ts0 = SCALE ? 1.0f / t.ts0 : 1.0f;
  const float sr = sqrtf(t.rot_weight), ss = SCALE ? sqrtf(t.scale_weight) : 0.f;
  for (int i = 0; i < 3; ++i)
  {
    r[i] = t.target[9 + i] * inv_ts0 - t10[i] * inv_s0;
    r[3 + i] = sr * (phit[i] - phi[i]);
  }
  r[6] = SCALE ? ss * (logf(t.ts1 / t.ts0) - logf(s1 / s0)) : 0.f;
  float e = 0.f;
  for (int i = 0; i < kGraphRows; ++i)
    e = fmaf(r[i], r[i], e);
  if (JAC)
  {
    for (int i = 0; i < kGraphRows; ++i)
      for (int j = 0; j < kGraphD; ++j)
        J[i][j] = 0.f;
    float Ji[3][3];
    so3_left_jacobian_inverse(phi, th2, Ji);
    // d t0 / d omega0 = e_j x t0 (column j)
    const float ext[3][3] = {{0.f, -t0[2], t0[1]}, {t0[2], 0.f, -t0[0]}, {-t0[1], t0[0], 0.f}};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
      {
        const float tv = R1[j * 3 + i] * inv_s0;                                                          // R1^T / s0
        const float tw = (R1[0 * 3 + i] * ext[j][0] + R1[1 * 3 + i] * ext[j][1] + R1[2 * 3 + i] * ext[j][2]) * inv_s0;
        const float rw = sr * (Ji[i][0] * R1[j * 3 + 0] + Ji[i][1] * R1[j * 3 + 1] + Ji[i][2] * R1[j * 3 + 2]); // Jl^-1 R1^T
        J[i][j] = tv;
        J[i][3 + j] = tw;
        J[3 + i][3 + j] = rw;
        J[i][6 + j] = -tv; // the pose1 block is minus the pose0 block
        J[i][9 + j] = -tw;
        J[3 + i][9 + j] = -rw;
      }
    if (SCALE)
    {
      for (int i = 0; i < 3; ++i)
        J[i][12] = -t10[i] * inv_s0 * inv_s0;
      J[6][12] = -ss * inv_s0;
      J[6][13] = ss / s1;
    }
  }
  return t.weight * e;
}

template <bool JAC>
SAGE_HD inline float graph_rel_pose_scale(const float *pose0, const float *pose1, float s0, float s1, const GraphTerm &t,
                                          float J[kGraphRows][kGraphD], float r[kGraphRows])
{
  return graph_rel_pose_body<true, JAC>(pose0, pose1, s0, s1, t, J, r);
}

template <bool JAC>
SAGE_HD inline float graph_rel_pose(const float *pose0, const float *pose1, const GraphTerm &t, float J[kGraphRows][kGraphD],
                                    float r[kGraphRows])
{
  return graph_rel_pose_body<false, JAC>(pose0, pose1, 1.0f, 1.0f, t, J, r);
}

// ScaleFactor against ts0: one residual (the last row) on the keyframe's scale, column 12
template <bool JAC>
SAGE_HD inline float graph_scale_prior(float s0, const GraphTerm &t, float J[kGraphRows][kGraphD], float r[kGraphRows])
{
  for (int i = 0; i < kGraphRows; ++i)
    r[i] = 0.f;
  r[6] = logf(t.ts0) - logf(s0);
  if (JAC)
  {
    for (int i = 0; i < kGraphRows; ++i)
      for (int j = 0; j < kGraphD; ++j)
        J[i][j] = 0.f;
    J[6][12] = 1.0f / s0;
  }
  return t.weight * (r[6] * r[6]);
}

// any kind
template <bool JAC>
SAGE_HD inline float graph_term_eval(const float *pose0, const float *pose1, float s0, float s1, const GraphTerm &t,
                                     float J[kGraphRows][kGraphD], float r[kGraphRows])
{
  if (t.kind == kGraphScalePrior)
    return graph_scale_prior<JAC>(s0, t, J, r);
  if (t.kind == kGraphRelPose)
    return graph_rel_pose<JAC>(pose0, pose1, t, J, r);
  return graph_rel_pose_scale<JAC>(pose0, pose1, s0, s1, t, J, r);
}

// AtA = weight * J^T J (row i), Atb = weight * J^T r (entry i): sums over the rows in a fixed order
SAGE_HD inline void graph_normal_row(const float J[kGraphRows][kGraphD], const float r[kGraphRows], float weight, int i,
                                     float AtA_row[kGraphD], float &Atb_i)
{
  float col[kGraphRows];
  for (int k = 0; k < kGraphRows; ++k)
  {
    col[k] = 0.f;
    for (int j = 0; j < kGraphD; ++j) // (a chain of selects: no dynamically indexed register array on the device)
      col[k] = (j == i) ? J[k][j] : col[k];
  }
  for (int j = 0; j < kGraphD; ++j)
  {
    float acc = 0.f;
    for (int k = 0; k < kGraphRows; ++k)
      acc = fmaf(col[k], J[k][j], acc);
    AtA_row[j] = weight * acc;
  }
  float acc = 0.f;
  for (int k = 0; k < kGraphRows; ++k)
    acc = fmaf(col[k], r[k], acc);
  Atb_i = weight * acc;
}

} // namespace sage
