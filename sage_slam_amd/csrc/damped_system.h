// damped_system.h -- the window's damped normal equations, its priors and its retraction, each written once for the
// device kernels (solve_kernels.hip) and the host code that mirrors them (window_solve.hip, block_solver.cpp,
// shard_solve.cpp, host_math.cpp).  Plain C++17, no HIP include: hipcc reads SAGE_HD as __host__ __device__, the host
// compiler as nothing.
//
//   A = H + P + damp * diag(H + P)     H: packed [K diag blocks | link blocks | gradient] (double), P: diagonal priors
//
// Held variables (sage_window_hold): a held row / column of A is the identity's -- no off-diagonal element in its diagonal
// block or its link blocks, diagonal 1, right-hand side 0, no prior -- so its delta is exactly zero and the free rows see
// the system with the held variables eliminated at their current values; the retraction copies held entries bit for bit.
// A group (pose, code, scale) that EVERY keyframe holds is not carried as identity rows at all: the system is built from the
// kept rows only (solver rows, below; which groups those are is window_plan.h's rule).
//
// The three builders of A's block storage keep their own iteration (per block on the device, per keyframe and per link
// with accumulation of duplicate links in sage_block_solve, local positions and ownership of priors in the shard); what
// an element is and where it goes is decided here.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define SAGE_HD __host__ __device__
#else
#define SAGE_HD
#endif

namespace sage
{

// ---- pose algebra (poses are 12 floats: R row-major, then t) ----

// gtsam_traits.h:78-89 : [t1 - R1 R0^T t0, log(R1 R0^T)]
SAGE_HD inline void pose_local(const float *origin, const float *other, double out[6])
{
  double Rr[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      Rr[i * 3 + j] = (double)other[i * 3 + 0] * origin[j * 3 + 0] + (double)other[i * 3 + 1] * origin[j * 3 + 1] +
                      (double)other[i * 3 + 2] * origin[j * 3 + 2];
  for (int i = 0; i < 3; ++i)
    out[i] = other[9 + i] - (Rr[i * 3 + 0] * origin[9] + Rr[i * 3 + 1] * origin[10] + Rr[i * 3 + 2] * origin[11]);
  const double tr = Rr[0] + Rr[4] + Rr[8];
  const double cs = fmin(1.0, fmax(-1.0, 0.5 * (tr - 1.0)));
  const double th = acos(cs);
  const double k = th < 1e-8 ? 0.5 : th / (2.0 * sin(th));
  out[3] = k * (Rr[7] - Rr[5]);
  out[4] = k * (Rr[2] - Rr[6]);
  out[5] = k * (Rr[3] - Rr[1]);
}

// mapping_utils.h:316-346 (fp32)
SAGE_HD inline void se3_exp(const float *omega, const float *v, float *R, float *t)
{
  float theta = sqrtf(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
  float n[3] = {1.f, 0.f, 0.f}; // "a casual rotation direction vector" when theta == 0
  if (theta > 0)
  {
    n[0] = omega[0] / theta;
    n[1] = omega[1] / theta;
    n[2] = omega[2] / theta;
  }
  theta = fmaxf(theta, 1.0e-14f);
  const float s = sinf(theta), c = cosf(theta);
  const float K[3][3] = {{0, -n[2], n[1]}, {n[2], 0, -n[0]}, {-n[1], n[0], 0}};
  float K2[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      K2[i][j] = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
  const float a = (1.0f - c) / theta, b = (theta - s) / theta;
  for (int i = 0; i < 3; ++i)
  {
    float acc = 0.f;
    for (int j = 0; j < 3; ++j)
    {
      const float id = (i == j) ? 1.f : 0.f;
      R[i * 3 + j] = id + s * K[i][j] + (1.0f - c) * K2[i][j];
      acc += (id + a * K[i][j] + b * K2[i][j]) * v[j];
    }
    t[i] = acc;
  }
}

// gtsam_traits.h:45-70, camera_tracker.cpp:491-512 : out = exp(d) * pose, d = [v, omega] (left update); out != pose
SAGE_HD inline void pose_retract(const float *pose, const float *d, float *out)
{
  float dR[9], dt[3];
  se3_exp(d + 3, d, dR, dt);
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j)
      out[i * 3 + j] = dR[i * 3 + 0] * pose[0 * 3 + j] + dR[i * 3 + 1] * pose[1 * 3 + j] + dR[i * 3 + 2] * pose[2 * 3 + j];
    out[9 + i] = dR[i * 3 + 0] * pose[9] + dR[i * 3 + 1] * pose[10] + dR[i * 3 + 2] * pose[11] + dt[i];
  }
}

// ---- held variables: a keyframe's mask of SAGE_HOLD_POSE = 1, SAGE_HOLD_CODE = 2, SAGE_HOLD_SCALE = 4 ----
enum : int { kHoldPose = 1, kHoldCode = 2, kHoldScale = 4, kHoldAll = 7 };

// is row r of a keyframe's block (rows: pose 6, code CS, scale) held under `hold`?
SAGE_HD inline bool row_held(int hold, int r, int CS)
{
  return (hold & (r < 6 ? kHoldPose : (r < 6 + CS ? kHoldCode : kHoldScale))) != 0;
}

// element (r, c) of a diagonal block where row r or column c is held
SAGE_HD inline double held_diag_elem(int r, int c) { return r == c ? 1.0 : 0.0; }

// ---- priors (a9): code prior on every keyframe (zero prior mean), scale / pose priors on keyframe 0 ----
struct SolvePriors
{
  double code_w, scale_w, pose_w;
  float scale_init0;
  float pose_init0[12];
};

// what the priors add to row r of keyframe kf (rows: pose 6, code CS, scale), given that keyframe's current variables:
// da on the diagonal of H, ga on the gradient; nothing on a row held under the keyframe's mask `hold`
SAGE_HD inline void prior_row(const SolvePriors &pri, int kf, int r, int CS, const float *pose, float scale,
                              const float *code, double &da, double &ga, int hold = 0)
{
  da = 0.0;
  ga = 0.0;
  if (hold && row_held(hold, r, CS))
    return;
  if (r >= 6 && r < 6 + CS)
  {
    da = pri.code_w;
    ga = pri.code_w * (0.0 - (double)code[r - 6]);
  }
  if (kf == 0 && r == 6 + CS && pri.scale_w > 0)
  {
    const double s = (double)scale;
    da = pri.scale_w / (s * s);
    ga = pri.scale_w / s * (log((double)pri.scale_init0) - log(s));
  }
  if (kf == 0 && r < 6 && pri.pose_w > 0)
  {
    double loc[6];
    pose_local(pose, pri.pose_init0, loc);
    da = pri.pose_w;
    ga = pri.pose_w * loc[r];
  }
}

// ---- element rules of the damped system ----

// element (r, c) of a keyframe's diagonal block: symmetrised, the prior and the LM damping H + damp*diag(H)
// (camera_tracker.cpp:1182) on the diagonal
SAGE_HD inline double damped_diag_elem(const double *D, int B, int r, int c, double prior, double damp)
{
  double v = 0.5 * (D[r * B + c] + D[c * B + r]);
  if (r == c)
    v = (v + prior) * (1.0 + damp);
  return v;
}

// the blocks are padded from B to Bp rows with a (damped) identity: delta 0 on the padding rows
SAGE_HD inline double damped_pad_elem(int r, int c, double damp) { return r == c ? 1.0 + damp : 0.0; }

SAGE_HD inline double damped_rhs_elem(double g, double g_prior) { return g + g_prior; }

// Blocks are stored transposed: element (r in the row keyframe, c in the column keyframe) at [c][r].
SAGE_HD inline int stored_slot(int r, int c, int Bp) { return c * Bp + r; }

// ... and comes from this element of the packed link block (a, b), a < b, which is [row in a][column in b]
SAGE_HD inline int link_elem(bool row_is_a, int r, int c, int B) { return row_is_a ? r * B + c : c * B + r; }

// ---- solver rows: a window in which every keyframe holds a whole group (window_plan.h: solver_rows) solves blocks of the
//      Bs kept rows only.  to_block[s] is the block row behind solver row s (null: every row is kept, s itself).  An element
//      of the compact system IS the element of the full system at the mapped rows -- the held rule, the symmetrisation, the
//      prior and the damping are those above, evaluated at block rows -- so the two builders below say only where to look.
SAGE_HD inline int block_row(const int *to_block, int s) { return to_block ? to_block[s] : s; }

// is element (solver row r of a keyframe held under hold_r, solver column c of one held under hold_c) a held one?
SAGE_HD inline bool solver_elem_held(int hold_r, int hold_c, const int *to_block, int r, int c, int CS)
{
  return (hold_r | hold_c) && (row_held(hold_r, block_row(to_block, r), CS) || row_held(hold_c, block_row(to_block, c), CS));
}

// element (r, c) in solver rows of a keyframe's diagonal block D [B x B]; prior: of block row to_block[r]
SAGE_HD inline double solver_diag_elem(const double *D, int B, const int *to_block, int r, int c, double prior, double damp)
{
  return damped_diag_elem(D, B, block_row(to_block, r), block_row(to_block, c), prior, damp);
}

// ... and where element (r in the row keyframe, c in the column keyframe) of a link block sits in the packed block [B x B]
SAGE_HD inline int solver_link_elem(bool row_is_a, const int *to_block, int r, int c, int B)
{
  return link_elem(row_is_a, block_row(to_block, r), block_row(to_block, c), B);
}

// the host builder: a packed system at B (the held rule already applied: hold_packed) and its prior vectors -> the packed
// system of the kept rows, [K diag | nlinks link | g] at Bs, and its priors [K][Bs].  Dropped rows are held rows: what is
// left behind is rows of the identity, nothing a kept row couples to.
inline void compact_packed(const double *packed, const double *dadd, const double *gadd, int K, int nlinks, int B, int Bs,
                           const int *to_block, double *packed_s, double *dadd_s, double *gadd_s)
{
  const size_t BB = (size_t)B * B, BBs = (size_t)Bs * Bs;
  const double *g = packed + (size_t)(K + nlinks) * BB;
  double *g_s = packed_s + (size_t)(K + nlinks) * BBs;
  for (int b = 0; b < K + nlinks; ++b) // diagonal and link blocks alike: [row][column], both through the map
    for (int r = 0; r < Bs; ++r)
      for (int c = 0; c < Bs; ++c)
        packed_s[b * BBs + (size_t)r * Bs + c] = packed[b * BB + (size_t)block_row(to_block, r) * B + block_row(to_block, c)];
  for (int k = 0; k < K; ++k)
    for (int r = 0; r < Bs; ++r)
    {
      const size_t from = (size_t)k * B + block_row(to_block, r), to = (size_t)k * Bs + r;
      g_s[to] = g[from];
      dadd_s[to] = dadd[from];
      gadd_s[to] = gadd[from];
    }
}

// ---- the held rule on a host copy of the packed system and its prior vectors, for the host block solve (the device
//      path applies the same element rules while it scatters): hold [K] masks, links [nlinks][2] ----
inline void hold_packed(double *packed, double *dadd, double *gadd, int K, int nlinks, const int *links, int B, int CS,
                        const unsigned char *hold)
{
  const int BB = B * B;
  double *lnk = packed + (size_t)K * BB, *g = lnk + (size_t)nlinks * BB;
  for (int k = 0; k < K; ++k)
  {
    if (!hold[k])
      continue;
    double *D = packed + (size_t)k * BB;
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c)
        if (row_held(hold[k], r, CS) || row_held(hold[k], c, CS))
          D[r * B + c] = held_diag_elem(r, c);
    for (int r = 0; r < B; ++r)
      if (row_held(hold[k], r, CS))
        g[(size_t)k * B + r] = dadd[(size_t)k * B + r] = gadd[(size_t)k * B + r] = 0.0;
  }
  for (int l = 0; l < nlinks; ++l)
  {
    const int ha = hold[links[2 * l]], hb = hold[links[2 * l + 1]];
    if (!ha && !hb)
      continue;
    for (int r = 0; r < B; ++r) // [row in a][column in b]
      for (int c = 0; c < B; ++c)
        if (row_held(ha, r, CS) || row_held(hb, c, CS))
          lnk[(size_t)l * BB + r * B + c] = 0.0;
  }
}

} // namespace sage
