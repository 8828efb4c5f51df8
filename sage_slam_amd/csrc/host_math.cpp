// host_math.cpp -- pure-CPU host helpers of the C ABI (no device needed).
//
//   sage_camera_pyramid      common/camera_pyramid.h:18-32 + pinhole_camera_impl.h:120-132
//   sage_se3_exp             core/mapping/mapping_utils.h:316-346
//   sage_pose_retract        core/gtsam/gtsam_traits.h:45-70, core/system/camera_tracker.cpp:491-512
//   sage_nearest_psd         the Higham algorithm core/mapping/mapping_utils.h:104-128 intends
//   sage_damped_solve_qr_f32 core/system/camera_tracker.cpp:1182-1183 (colPivHouseholderQr in fp32)
//   sage_track_lm            core/system/camera_tracker.cpp:1156-1279 (+ LMConvergence :527-573)
#include <algorithm>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <numeric>
#include <random>
#include <vector>

#include "damped_system.h"
#include "host_math.h"
#include "sage_ba.h"

extern "C" const char *sage_version(void) { return "sage-ba-mi355x 0.1 (gfx950)"; }

extern "C" const char *sage_error_string(int code)
{
  switch (code)
  {
  case SAGE_OK:
    return "ok";
  case SAGE_E_INVALID:
    return "invalid argument";
  case SAGE_E_UNSUPPORTED:
    return "unsupported CS/FS/levels combination";
  case SAGE_E_NOT_PSD:
    return "normal equations not positive definite";
  case SAGE_E_STATE:
    return "call order violated";
  case SAGE_E_NO_OVERLAP:
    return "tracker: no overlap between the frame to track and the keyframe";
  default:
    return code > 0 ? "HIP runtime error (hipError_t)" : "unknown error";
  }
}

extern "C" int sage_camera_pyramid(const SageCamera *base, int levels, SagePyramid *out)
{
  if (!base || !out || levels < 1 || levels > SAGE_MAX_LEVELS)
    return SAGE_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  out->levels = levels;
  int off = 0;
  for (int i = 0; i < levels; ++i)
  {
    SageCamera c = (i == 0) ? *base : out->cam[i - 1];
    if (i != 0)
    {
      // new size = (size_t)(w/2), (size_t)(h/2); fx,u0 *= new_w/w ; fy,v0 *= new_h/h   (all fp32)
      const size_t nw = (size_t)(c.w / 2), nh = (size_t)(c.h / 2);
      const float xr = (float)nw / c.w, yr = (float)nh / c.h;
      c.fx *= xr;
      c.fy *= yr;
      c.cx *= xr;
      c.cy *= yr;
      c.w = (float)nw;
      c.h = (float)nh;
    }
    out->cam[i] = c;
    out->level_offsets[i] = off;
    off += (int)c.w * (int)c.h;
  }
  out->P = off;
  return SAGE_OK;
}

// mapper.cpp:1326-1333: the keyframe's sample permutation (the reference's own standard-library calls)
extern "C" int sage_shuffle_indices(int64_t seed, int64_t n, int64_t *idx)
{
  if (n < 0 || (n > 0 && !idx))
    return SAGE_E_INVALID;
  std::vector<long> indices((size_t)n);
  std::iota(indices.begin(), indices.end(), 0);
  std::mt19937 g;
  g.seed((long)seed);
  std::shuffle(indices.begin(), indices.end(), g);
  for (int64_t i = 0; i < n; ++i)
    idx[i] = indices[(size_t)i];
  return SAGE_OK;
}

extern "C" void sage_se3_exp(const float *omega, const float *v, float *R, float *t)
{
  if (!omega || !v || !R || !t) // (void helpers: a null argument is a no-op, never a fault)
    return;
  sage::se3_exp(omega, v, R, t);
}

extern "C" void sage_pose_retract(const float *pose, const float *d, float *out)
{
  if (!pose || !d || !out)
    return;
  float o[12]; // (out may be pose)
  sage::pose_retract(pose, d, o); // delta = [v, omega]
  std::memcpy(out, o, sizeof(o));
}

// ---------------------------------------------------------------- dense helpers (double)
namespace sage
{

// cyclic Jacobi eigen-decomposition of a symmetric matrix: A = V diag(w) V^T (columns of V)
void sym_eig(std::vector<double> &A, int n, std::vector<double> &w, std::vector<double> &V)
{
  V.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    V[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep)
  {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        (i == j ? diag : off) += A[(size_t)i * n + j] * A[(size_t)i * n + j];
    if (off <= 1e-30 * (diag + 1e-300))
      break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q)
      {
        const double apq = A[(size_t)p * n + q];
        if (std::fabs(apq) < 1e-300)
          continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        const double tau = (aqq - app) / (2.0 * apq);
        const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        for (int k = 0; k < n; ++k)
        {
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - s * akq;
          A[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k)
        {
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - s * aqk;
          A[(size_t)q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k)
        {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = c * vkp - s * vkq;
          V[(size_t)k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  w.resize(n);
  for (int i = 0; i < n; ++i)
    w[i] = A[(size_t)i * n + i];
}

// Symmetric eigen-decomposition by Householder tridiagonalisation + implicit QL (the EISPACK tred2 / tql2 pair): the same
// A = V diag(w) V^T as sym_eig at ~1/15 of the time for the 45 x 45 / 78 x 78 factor matrices (Higham projection of
// sage_nearest_psd: the per-factor host cost of the gtsam path).  Returns false if QL does not converge (the caller falls
// back to the Jacobi sweeps).  A is destroyed.
// (SAGE_HOT: starts on a 64-byte line.  Its loops run 4-7 % slower or faster with where they fall in a line, and a function
// aligned to 16 bytes moves whenever a unit linked in front of it changes size)
#define SAGE_HOT __attribute__((aligned(64)))
SAGE_HOT static bool sym_eig_ql(std::vector<double> &A, int n, std::vector<double> &w, std::vector<double> &V)
{
  std::vector<double> e(n, 0.0);
  w.assign(n, 0.0);
  auto a = [&](int i, int j) -> double & { return A[(size_t)i * n + j]; };
  for (int i = n - 1; i >= 1; --i)
  {
    const int l = i - 1;
    double h = 0.0, scale = 0.0;
    if (l > 0)
    {
      for (int k = 0; k <= l; ++k)
        scale += std::fabs(a(i, k));
      if (scale == 0.0)
        e[i] = a(i, l);
      else
      {
        for (int k = 0; k <= l; ++k)
        {
          a(i, k) /= scale;
          h += a(i, k) * a(i, k);
        }
        double f = a(i, l);
        double g = f >= 0.0 ? -std::sqrt(h) : std::sqrt(h);
        e[i] = scale * g;
        h -= f * g;
        a(i, l) = f - g;
        f = 0.0;
        for (int j = 0; j <= l; ++j)
        {
          a(j, i) = a(i, j) / h;
          g = 0.0;
          for (int k = 0; k <= j; ++k)
            g += a(j, k) * a(i, k);
          for (int k = j + 1; k <= l; ++k)
            g += a(k, j) * a(i, k);
          e[j] = g / h;
          f += e[j] * a(i, j);
        }
        const double hh = f / (h + h);
        for (int j = 0; j <= l; ++j)
        {
          f = a(i, j);
          e[j] = g = e[j] - hh * f;
          for (int k = 0; k <= j; ++k)
            a(j, k) -= f * e[k] + g * a(i, k);
        }
      }
    }
    else
      e[i] = a(i, l);
    w[i] = h;
  }
  w[0] = 0.0;
  e[0] = 0.0;
  for (int i = 0; i < n; ++i)
  {
    const int l = i - 1;
    if (w[i] != 0.0)
      for (int j = 0; j <= l; ++j)
      {
        double g = 0.0;
        for (int k = 0; k <= l; ++k)
          g += a(i, k) * a(k, j);
        for (int k = 0; k <= l; ++k)
          a(k, j) -= g * a(k, i);
      }
    w[i] = a(i, i);
    a(i, i) = 1.0;
    for (int j = 0; j <= l; ++j)
      a(j, i) = a(i, j) = 0.0;
  }
  // rows of Z = the accumulated transformation transposed: the QL rotations then touch two contiguous rows
  std::vector<double> Z((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k)
      Z[(size_t)i * n + k] = a(k, i);
  for (int i = 1; i < n; ++i)
    e[i - 1] = e[i];
  e[n - 1] = 0.0;
  const double eps = std::numeric_limits<double>::epsilon();
  for (int l = 0; l < n; ++l)
  {
    int iter = 0, m;
    do
    {
      for (m = l; m < n - 1; ++m)
      {
        const double dd = std::fabs(w[m]) + std::fabs(w[m + 1]);
        if (std::fabs(e[m]) <= eps * dd)
          break;
      }
      if (m != l)
      {
        if (iter++ == 80)
          return false;
        double g = (w[l + 1] - w[l]) / (2.0 * e[l]);
        double r = std::hypot(g, 1.0);
        g = w[m] - w[l] + e[l] / (g + (g >= 0.0 ? std::fabs(r) : -std::fabs(r)));
        double sn = 1.0, cs = 1.0, pp = 0.0;
        int i;
        for (i = m - 1; i >= l; --i)
        {
          double f = sn * e[i];
          const double b = cs * e[i];
          e[i + 1] = (r = std::hypot(f, g));
          if (r == 0.0)
          {
            w[i + 1] -= pp;
            e[m] = 0.0;
            break;
          }
          sn = f / r;
          cs = g / r;
          g = w[i + 1] - pp;
          r = (w[i] - g) * sn + 2.0 * cs * b;
          w[i + 1] = g + (pp = sn * r);
          g = cs * r - b;
          double *zi = &Z[(size_t)i * n], *zj = &Z[(size_t)(i + 1) * n];
          for (int k = 0; k < n; ++k)
          {
            f = zj[k];
            zj[k] = sn * zi[k] + cs * f;
            zi[k] = cs * zi[k] - sn * f;
          }
        }
        if (r == 0.0 && i >= l)
          continue;
        w[l] -= pp;
        e[l] = g;
        e[m] = 0.0;
      }
    } while (m != l);
  }
  V.resize((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k)
      V[(size_t)k * n + i] = Z[(size_t)i * n + k];
  return true;
}

// sum_k a[k] * b[k] with four independent partial sums (strict fp semantics keep the compiler from splitting one chain)
static inline double dot4(const double *a, const double *b, int n)
{
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int k = 0;
  for (; k + 4 <= n; k += 4)
  {
    s0 += a[k] * b[k];
    s1 += a[k + 1] * b[k + 1];
    s2 += a[k + 2] * b[k + 2];
    s3 += a[k + 3] * b[k + 3];
  }
  for (; k < n; ++k)
    s0 += a[k] * b[k];
  return (s0 + s1) + (s2 + s3);
}

// LDLT-style positive (semi-)definiteness test (Eigen::LDLT::isPositive): all pivots >= 0.
static bool is_psd(const std::vector<double> &M, int n)
{
  std::vector<double> L(M), Ld((size_t)n * n, 0.0); // Ld[j][k] = L[j][k] * d_k: every inner sum is a contiguous dot product
  for (int j = 0; j < n; ++j)
  {
    const double d = L[(size_t)j * n + j] - dot4(&L[(size_t)j * n], &Ld[(size_t)j * n], j);
    if (d < 0.0)
      return false;
    L[(size_t)j * n + j] = d;
    for (int i = j + 1; i < n; ++i)
    {
      const double sv = L[(size_t)i * n + j] - dot4(&L[(size_t)i * n], &Ld[(size_t)j * n], j);
      const double lij = (d != 0.0) ? sv / d : 0.0;
      L[(size_t)i * n + j] = lij;
      Ld[(size_t)i * n + j] = lij * d;
    }
  }
  return true;
}

} // namespace sage

extern "C" SAGE_HOT int sage_nearest_psd(const double *M, int n, double *out)
{
  if (!M || !out || n < 1)
    return SAGE_E_INVALID;
  // B = (M + M^T)/2 ; H = polar factor of B = V |Lambda| V^T ; A2 = (B+H)/2 ; A3 = sym(A2)
  std::vector<double> B((size_t)n * n), w, V;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      B[(size_t)i * n + j] = 0.5 * (M[(size_t)i * n + j] + M[(size_t)j * n + i]);
  std::vector<double> tmp(B);
  if (!sage::sym_eig_ql(tmp, n, w, V))
  {
    tmp = B;
    sage::sym_eig(tmp, n, w, V);
  }
  std::vector<double> A3((size_t)n * n, 0.0), VW((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k)
      VW[(size_t)i * n + k] = V[(size_t)i * n + k] * std::fabs(w[k]);
  for (int i = 0; i < n; ++i)
    for (int j = i; j < n; ++j) // H = V |Lambda| V^T is symmetric: one triangle, mirrored (= the symmetrisation of A2)
    {
      const double h = sage::dot4(&VW[(size_t)i * n], &V[(size_t)j * n], n);
      A3[(size_t)i * n + j] = A3[(size_t)j * n + i] = 0.5 * (B[(size_t)i * n + j] + h);
    }
  // bump by (-min_eig*k + spacing) until LDLT-positive (mapping_utils.h:119-126).  The eigenvalues of A3 + c I are those
  // of A3 plus c: ONE decomposition serves every round of the loop.
  double k = 1; // (a double: 60 doublings of an int would overflow)
  const double spacing = 1e-15;
  bool have_min = false;
  double mn = 0.0;
  for (int it = 0; it < 60 && !sage::is_psd(A3, n); ++it)
  {
    if (!have_min)
    {
      std::vector<double> t2(A3), w2, V2;
      if (!sage::sym_eig_ql(t2, n, w2, V2))
      {
        t2 = A3;
        sage::sym_eig(t2, n, w2, V2);
      }
      mn = *std::min_element(w2.begin(), w2.end());
      have_min = true;
    }
    // a bump below the rounding granularity of the diagonal would move the tracked minimum but not the matrix: never
    // less than one ulp of the largest diagonal entry, and never negative (the tracked minimum turns positive after the
    // first round; the matrix is re-measured then instead of being walked back)
    double dmax = 0.0;
    for (int i = 0; i < n; ++i)
      dmax = std::max(dmax, std::fabs(A3[(size_t)i * n + i]));
    const double ulp = dmax * 2.220446049250313e-16;
    double bump = -mn * k + spacing;
    if (bump < ulp)
    {
      if (mn > 0.0) // the estimate says PSD but the LDLT test disagrees: measure again on the matrix as it is now
        have_min = false;
      bump = ulp;
    }
    for (int i = 0; i < n; ++i)
      A3[(size_t)i * n + i] += bump;
    mn += bump;
    k *= 2;
  }
  std::memcpy(out, A3.data(), sizeof(double) * n * n);
  return SAGE_OK;
}

// ---------------------------------------------------------------- NearestPsd exactly as the reference wrote it
namespace sage
{
// Two-sided Jacobi SVD of a square real matrix the way Eigen 3.3.9's JacobiSVD runs it (the reference's
// `Eigen::JacobiSVD<T> svd(B, ComputeThinV)`, mapping_utils.h:111): work = B / max|B|; sweeps over (p, q < p) while any
// off-diagonal pair exceeds max(DBL_MIN, 2 eps * max diagonal); each pair: a left rotation that symmetrises the 2x2
// block, then a symmetric Jacobi rotation on both sides; |diagonal| = singular values sorted descending with the columns
// of V swapped alongside.  Only V (what `matrixV()` returns) and sigma are produced.  The point of restating the
// procedure instead of calling any SVD: the reference's  H = V^T diag(sigma) V  is NOT invariant under the sign / order
// conventions of V, so it can only be reproduced by walking the same rotations.
static void eigen_jacobi_svd_v(const std::vector<double> &B, int n, std::vector<double> &V, std::vector<double> &sv)
{
  double scale = 0.0;
  for (double v : B)
    scale = std::max(scale, std::fabs(v));
  if (scale == 0.0)
    scale = 1.0;
  std::vector<double> Wk(B);
  for (double &v : Wk)
    v /= scale;
  V.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
    V[(size_t)i * n + i] = 1.0;
  auto W = [&](int i, int j) -> double & { return Wk[(size_t)i * n + j]; };
  const double tiny = std::numeric_limits<double>::min(), prec = 2.0 * std::numeric_limits<double>::epsilon();
  double max_diag = 0.0;
  for (int i = 0; i < n; ++i)
    max_diag = std::max(max_diag, std::fabs(W(i, i)));
  bool finished = false;
  while (!finished)
  {
    finished = true;
    for (int p = 1; p < n; ++p)
      for (int q = 0; q < p; ++q)
      {
        const double thr = std::max(tiny, prec * max_diag);
        if (!(std::fabs(W(p, q)) > thr || std::fabs(W(q, p)) > thr))
          continue;
        finished = false;
        // 2x2 block [[W(p,p), W(p,q)], [W(q,p), W(q,q)]]: rot1 makes it symmetric ...
        double m00 = W(p, p), m01 = W(p, q), m10 = W(q, p), m11 = W(q, q);
        double c1, s1;
        {
          const double t = m00 + m11, d = m10 - m01;
          if (std::fabs(d) < tiny)
          {
            s1 = 0.0;
            c1 = 1.0;
          }
          else
          {
            const double u = t / d, tmp = std::sqrt(1.0 + u * u);
            s1 = 1.0 / tmp;
            c1 = u / tmp;
          }
        }
        {
          const double a0 = c1 * m00 + s1 * m10, a1 = c1 * m01 + s1 * m11;
          const double b0 = -s1 * m00 + c1 * m10, b1 = -s1 * m01 + c1 * m11;
          m00 = a0; m01 = a1; m10 = b0; m11 = b1;
        }
        // ... j_right diagonalises the symmetric block (makeJacobi(x = m00, y = m01, z = m11))
        double cr, sr;
        {
          const double deno = 2.0 * std::fabs(m01);
          if (deno < tiny)
          {
            cr = 1.0;
            sr = 0.0;
          }
          else
          {
            const double tau = (m00 - m11) / deno, w = std::sqrt(tau * tau + 1.0);
            const double t = tau > 0.0 ? 1.0 / (tau + w) : 1.0 / (tau - w);
            const double sign_t = t > 0.0 ? 1.0 : -1.0, nn = 1.0 / std::sqrt(t * t + 1.0);
            sr = -sign_t * (m01 / std::fabs(m01)) * std::fabs(t) * nn;
            cr = nn;
          }
        }
        // j_left = rot1 * j_right^T
        const double cl = c1 * cr + s1 * sr, sl = -c1 * sr + s1 * cr;
        for (int k = 0; k < n; ++k) // rows p, q from the left
        {
          const double x = W(p, k), y = W(q, k);
          W(p, k) = cl * x + sl * y;
          W(q, k) = -sl * x + cl * y;
        }
        for (int k = 0; k < n; ++k) // columns p, q from the right (work matrix and V)
        {
          const double x = W(k, p), y = W(k, q);
          W(k, p) = cr * x - sr * y;
          W(k, q) = sr * x + cr * y;
          const double vx = V[(size_t)k * n + p], vy = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = cr * vx - sr * vy;
          V[(size_t)k * n + q] = sr * vx + cr * vy;
        }
        max_diag = std::max(max_diag, std::max(std::fabs(W(p, p)), std::fabs(W(q, q))));
      }
  }
  sv.resize(n);
  for (int i = 0; i < n; ++i)
    sv[i] = std::fabs(W(i, i)) * scale; // (negative diagonals flip columns of U, which the reference never asks for)
  for (int i = 0; i < n; ++i)
  {
    int pos = i;
    for (int j = i + 1; j < n; ++j)
      if (sv[j] > sv[pos])
        pos = j;
    if (sv[pos] == 0.0)
      break;
    if (pos != i)
    {
      std::swap(sv[i], sv[pos]);
      for (int k = 0; k < n; ++k)
        std::swap(V[(size_t)k * n + i], V[(size_t)k * n + pos]);
    }
  }
}

// Eigen::LDLT::isPositive(): the pivoted LDL^T (largest remaining |diagonal| first) meets no negative pivot
static bool eigen_ldlt_is_positive(const std::vector<double> &M, int n)
{
  std::vector<double> A(M);
  auto a = [&](int i, int j) -> double & { return A[(size_t)i * n + j]; };
  for (int k = 0; k < n; ++k)
  {
    int piv = k;
    for (int i = k + 1; i < n; ++i)
      if (std::fabs(a(i, i)) > std::fabs(a(piv, piv)))
        piv = i;
    if (piv != k)
    {
      for (int j = 0; j < n; ++j)
        std::swap(a(k, j), a(piv, j));
      for (int i = 0; i < n; ++i)
        std::swap(a(i, k), a(i, piv));
    }
    const double d = a(k, k);
    if (d < 0.0)
      return false;
    if (d == 0.0)
      continue;
    for (int i = k + 1; i < n; ++i)
    {
      const double l = a(i, k) / d;
      for (int j = k + 1; j < n; ++j)
        a(i, j) -= l * a(k, j);
    }
  }
  return true;
}
} // namespace sage

extern "C" int sage_nearest_psd_reference(const double *M, int n, double *out)
{
  if (!M || !out || n < 1)
    return SAGE_E_INVALID;
  std::vector<double> B((size_t)n * n), V, sv;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      B[(size_t)i * n + j] = (M[(size_t)i * n + j] + M[(size_t)j * n + i]) / 2;
  sage::eigen_jacobi_svd_v(B, n, V, sv);
  // H = V^T diag(sigma) V  (mapping_utils.h:112, as written): H_ij = sum_k sigma_k V_ki V_kj
  std::vector<double> A3((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
    {
      double h = 0.0;
      for (int k = 0; k < n; ++k)
        h += V[(size_t)k * n + i] * sv[k] * V[(size_t)k * n + j];
      A3[(size_t)i * n + j] = (B[(size_t)i * n + j] + h) / 2;
    }
  std::vector<double> S(A3);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      A3[(size_t)i * n + j] = (S[(size_t)i * n + j] + S[(size_t)j * n + i]) / 2;
  double k = 1; // (a double: 60 doublings of an int would overflow)
  const double spacing = 1e-15;
  for (int it = 0; it < 60 && !sage::eigen_ldlt_is_positive(A3, n); ++it)
  {
    std::vector<double> t2(A3), w2, V2;
    sage::sym_eig(t2, n, w2, V2);
    const double mn = *std::min_element(w2.begin(), w2.end());
    for (int i = 0; i < n; ++i)
      A3[(size_t)i * n + i] += -mn * k + spacing;
    k *= 2;
  }
  std::memcpy(out, A3.data(), sizeof(double) * n * n);
  return SAGE_OK;
}

extern "C" int sage_damped_solve_qr_f32(const float *A, const float *b, int n, float damp, float *x)
{
  if (!A || !b || !x || n < 1 || n > 64)
    return SAGE_E_INVALID;
  // (AtA + damp*diag(AtA)).colPivHouseholderQr().solve(Atb) in fp32 (camera_tracker.cpp:1182-1183), restated after Eigen
  // 3.3.9 step by step so that the RANK DECISION is Eigen's: ColPivHouseholderQR::computeInPlace (ColPivHouseholderQR.h:
  // 480-570) pivots on DOWNDATED column norms (LAPACK xGEQPF rule, recomputed when the downdate loses accuracy), counts
  // m_nonzero_pivots = the first k whose largest remaining squared norm is < (eps * max initial norm)^2 / rows * (rows-k),
  // makeHouseholderInPlace's (tau, beta) convention (Householder.h:65-93), and _solve_impl (:589-610): only the first
  // nonzero_pivots reflectors touch the right-hand side, the leading triangle is solved, the other components are zero.
  // Pinned by tests/golden/colpiv_qr_eigen339.json (produced with the vendored Eigen).  Column-major like Eigen.
  const float eps = std::numeric_limits<float>::epsilon();
  std::vector<float> M((size_t)n * n), c(b, b + n), hco(n, 0.f), upd(n), dir(n), tmp(n);
  auto at = [&](int i, int j) -> float & { return M[(size_t)j * n + i]; };
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      at(i, j) = A[(size_t)i * n + j] + (i == j ? damp * A[(size_t)i * n + i] : 0.f);
  auto col_norm = [&](int j, int from) {
    float sq = 0.f;
    for (int i = from; i < n; ++i)
      sq += at(i, j) * at(i, j);
    return std::sqrt(sq);
  };
  float maxcol = 0.f;
  for (int j = 0; j < n; ++j)
  {
    dir[j] = upd[j] = col_norm(j, 0);
    maxcol = std::max(maxcol, upd[j]);
  }
  const float thr_helper = (maxcol * eps) * (maxcol * eps) / (float)n;
  const float downdate_thr = std::sqrt(eps);
  std::vector<int> transp(n);
  int rank = n;
  for (int k = 0; k < n; ++k)
  {
    int best = k;
    for (int j = k + 1; j < n; ++j) // maxCoeff: the first maximal entry
      if (upd[j] > upd[best])
        best = j;
    const float biggest_sq = upd[best] * upd[best];
    if (rank == n && biggest_sq < thr_helper * (float)(n - k))
      rank = k;
    transp[k] = best;
    if (best != k)
    {
      for (int i = 0; i < n; ++i)
        std::swap(at(i, k), at(i, best));
      std::swap(upd[k], upd[best]);
      std::swap(dir[k], dir[best]);
    }
    // makeHouseholderInPlace on column k, rows k..n-1
    float tail_sq = 0.f;
    for (int i = k + 1; i < n; ++i)
      tail_sq += at(i, k) * at(i, k);
    const float c0 = at(k, k);
    float tau, beta;
    if (tail_sq <= std::numeric_limits<float>::min())
    {
      tau = 0.f;
      beta = c0;
      for (int i = k + 1; i < n; ++i)
        at(i, k) = 0.f;
    }
    else
    {
      beta = std::sqrt(c0 * c0 + tail_sq);
      if (c0 >= 0.f)
        beta = -beta;
      for (int i = k + 1; i < n; ++i)
        at(i, k) /= (c0 - beta);
      tau = (beta - c0) / beta;
    }
    hco[k] = tau;
    at(k, k) = beta;
    // applyHouseholderOnTheLeft to the trailing columns
    if (n - k == 1)
    { /* no trailing block */ }
    else if (tau != 0.f)
      for (int j = k + 1; j < n; ++j)
      {
        float t = 0.f;
        for (int i = k + 1; i < n; ++i)
          t += at(i, k) * at(i, j);
        t += at(k, j);
        at(k, j) -= tau * t;
        for (int i = k + 1; i < n; ++i)
          at(i, j) -= tau * at(i, k) * t;
      }
    for (int j = k + 1; j < n; ++j)
      if (upd[j] != 0.f)
      {
        float t = std::fabs(at(k, j)) / upd[j];
        t = (1.f + t) * (1.f - t);
        t = t < 0.f ? 0.f : t;
        const float q = upd[j] / dir[j];
        const float t2 = t * (q * q);
        if (t2 <= downdate_thr)
          dir[j] = upd[j] = col_norm(j, k + 1);
        else
          upd[j] *= std::sqrt(t);
      }
  }
  std::vector<int> perm(n);
  for (int i = 0; i < n; ++i)
    perm[i] = i;
  for (int k = 0; k < n; ++k)
    std::swap(perm[k], perm[transp[k]]);
  for (int i = 0; i < n; ++i)
    x[i] = 0.f;
  if (rank == 0)
    return SAGE_OK;
  for (int k = 0; k < rank; ++k) // c = H_{rank-1} ... H_0 c
  {
    if (hco[k] == 0.f)
      continue;
    float t = c[k];
    for (int i = k + 1; i < n; ++i)
      t += at(i, k) * c[i];
    c[k] -= hco[k] * t;
    for (int i = k + 1; i < n; ++i)
      c[i] -= hco[k] * at(i, k) * t;
  }
  for (int i = rank - 1; i >= 0; --i)
  {
    float t = c[i];
    for (int j = i + 1; j < rank; ++j)
      t -= at(i, j) * tmp[j];
    tmp[i] = t / at(i, i);
  }
  for (int i = 0; i < rank; ++i)
    x[perm[i]] = tmp[i];
  return SAGE_OK;
}

// ---------------------------------------------------------------- tracker LM policy
extern "C" void sage_lm_config_default(SageLmConfig *c)
{
  if (!c)
    return;
  // system/configs/slam_run.flags:17-23
  c->max_num_iters = 40;
  c->min_grad_thresh = 1.0e-4f;
  c->min_param_inc_thresh = 1.0e-2f;
  c->init_damp = 1.0e-4f;
  c->min_damp = 1.0e-6f;
  c->max_damp = 1.0e-2f;
  c->damp_dec_factor = 10.f;
  c->damp_inc_factor = 100.f;
  c->jac_update_err_inc_threshold = 1.0e-2f;
  c->max_inner_evals = 0;
  c->no_overlap_error = 0.f;
  c->linearize_at_candidate = 0;
}

namespace sage
{

// RotationToAngleAxis(R, 1e-6) as written in core/mapping/mapping_utils.h:143-212, including its quirks:
// the returned vector uses the HALF angle atan2(sin, cos) (the "2.0 *" of the torchgeometry original is
// missing) and case c0 divides by sqrt(0).  Only used by the convergence test.
void rotation_to_angle_axis_as_reference(const float *R, float eps, float *out)
{
  // rmat_t = R^T
  auto rt = [&](int i, int j) { return R[j * 3 + i]; };
  const bool d2 = rt(2, 2) < eps;
  const bool d0_d1 = rt(0, 0) > rt(1, 1);
  const bool d0_nd1 = rt(0, 0) < -rt(1, 1);
  const float t0 = 1.0f + rt(0, 0) - rt(1, 1) - rt(2, 2);
  const float t1 = 1.0f - rt(0, 0) + rt(1, 1) - rt(2, 2);
  const float t2 = 1.0f - rt(0, 0) - rt(1, 1) + rt(2, 2);
  const float t3 = 1.0f + rt(0, 0) + rt(1, 1) + rt(2, 2);
  float q[4], den;
  if (d2 && d0_d1)
  {
    q[0] = rt(1, 2) - rt(2, 1); q[1] = t0; q[2] = rt(0, 1) + rt(1, 0); q[3] = rt(2, 0) + rt(0, 2);
    den = 0.f; // t0*mask_c1 (sic) -> 0 in case c0
  }
  else if (d2)
  {
    q[0] = rt(2, 0) - rt(0, 2); q[1] = rt(0, 1) + rt(1, 0); q[2] = t1; q[3] = rt(1, 2) + rt(2, 1);
    den = t0 + t1; // t0*mask_c1 + t1*mask_c1 (sic)
  }
  else if (d0_nd1)
  {
    q[0] = rt(0, 1) - rt(1, 0); q[1] = rt(2, 0) + rt(0, 2); q[2] = rt(1, 2) + rt(2, 1); q[3] = t2;
    den = t2;
  }
  else
  {
    q[0] = t3; q[1] = rt(1, 2) - rt(2, 1); q[2] = rt(2, 0) - rt(0, 2); q[3] = rt(0, 1) - rt(1, 0);
    den = t3;
  }
  const float sq = std::sqrt(den);
  for (int i = 0; i < 4; ++i)
    q[i] = 0.5f * q[i] / sq;
  const float ss = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  const float sn = std::sqrt(ss), cs = q[0];
  const float two_theta = cs < 0.0f ? std::atan2(-sn, -cs) : std::atan2(sn, cs);
  const float k = ss > 0.0f ? two_theta / sn : 2.0f;
  out[0] = k * q[1];
  out[1] = k * q[2];
  out[2] = k * q[3];
}

static bool lm_converged(const SageLmConfig &cfg, int dof, const float *pose, float scale, const float *Atb,
                         const float *sol)
{
  float rv[3];
  rotation_to_angle_axis_as_reference(pose, 1.0e-6f, rv);
  float max_grad = 0.f;
  for (int i = 0; i < dof; ++i)
    max_grad = std::max(max_grad, std::fabs(Atb[i]));
  // max( solution / (|[t, rotvec, scale]| + 1e-8) ) -- signed numerator, as written (:531-536)
  const float den[7] = {std::fabs(pose[9]), std::fabs(pose[10]), std::fabs(pose[11]),
                        std::fabs(rv[0]), std::fabs(rv[1]), std::fabs(rv[2]), std::fabs(scale)};
  float max_inc = -INFINITY;
  bool nan = false;
  for (int i = 0; i < dof; ++i)
  {
    const float r = sol[i] / (den[i] + 1.0e-8f);
    if (r != r)
      nan = true;
    max_inc = std::max(max_inc, r);
  }
  if (nan)
    max_inc = NAN;
  return max_grad < cfg.min_grad_thresh || max_inc < cfg.min_param_inc_thresh;
}

} // namespace sage

namespace sage
{

// The tracker's LM policy (camera_tracker.cpp:1156-1279) as a resumable stepper: the state is what the reference's loop keeps
// between two evaluations, and the loop's body is cut where it evaluates.  start() and feed() answer with what the policy
// needs next -- the linearisation at (req_pose, req_scale), the error there, or nothing more (done, `status`) -- and feed()
// takes the answer.  sage_track_lm drives one stepper with its two callbacks, sage_track_lm_batch B of them in lock-step:
// one definition of the policy.
struct LmStepper
{
  enum Ask { kLinearize, kError, kDone };
  SageLmConfig cfg;
  int dof = 6;
  float AtA[49], Atb[7], sol[7];
  float guess[12], cand[12];
  float guess_scale = 1.f, cand_scale = 1.f;
  bool update_jac = true;
  float prev_error = 0.f, curr_error = 1.f, cand_error = 0.f;
  long curr_iter = 0;
  float damp = 0.f;
  SageLmTraceEntry *trace = nullptr;
  int trace_cap = 0, ntrace = 0;
  Ask ask = kDone;
  int status = 0;    // done: SAGE_OK or SAGE_E_NO_OVERLAP; `failed`: the code of the damped solve
  bool failed = false; // done on a failed solve: the caller returns `status` and writes no outputs
  const float *req_pose = nullptr;
  float req_scale = 1.f;

  void init(const SageLmConfig &c, int dof_, const float *pose12, const float *scale, SageLmTraceEntry *tr, int cap)
  {
    cfg = c;
    dof = dof_;
    for (int i = 0; i < 7; ++i)
      sol[i] = 0.f;
    std::memcpy(guess, pose12, sizeof(guess));
    guess_scale = scale ? *scale : 1.0f;
    cand_scale = guess_scale;
    damp = cfg.init_damp;
    trace = tr;
    trace_cap = cap;
  }
  float clampd(float d) const { return std::min(std::max(cfg.min_damp, d), cfg.max_damp); }
  Ask done(int st, bool fail = false)
  {
    status = st;
    failed = fail;
    return ask = kDone;
  }
  Ask want(Ask what, const float *pose, float scale)
  {
    req_pose = pose;
    req_scale = scale;
    return ask = what;
  }
  Ask start() { return top(); }
  // the answer to the last request.  kLinearize: A [dof x dof], b [dof] (may be this stepper's own AtA / Atb) and the error;
  // kError: the error alone
  Ask feed(const float *A, const float *b, float error)
  {
    if (ask == kLinearize)
    {
      if (A != AtA)
        std::memcpy(AtA, A, sizeof(float) * dof * dof);
      if (b != Atb)
        std::memcpy(Atb, b, sizeof(float) * dof);
      if (curr_iter == 0) // update_error only on the first pass (:1166, :1491); later the accepted candidate's error stands
        curr_error = error;
      update_jac = true;
      return after_linearize();
    }
    if (ask != kError)
      return ask;
    cand_error = error;
    if (cand_error < curr_error)
      return after_inner(true);
    if (damp < cfg.max_damp) // the inner damping retry
    {
      damp = clampd(damp * cfg.damp_inc_factor);
      const int rc = sage_damped_solve_qr_f32(AtA, Atb, dof, damp, sol);
      if (rc != 0)
        return done(rc, true);
      return propose();
    }
    return after_inner(false);
  }

private:
  Ask top()
  {
    // skip the Jacobian when the last step changed the error too little (:1159): from accept straight to the next solve
    if (std::fabs(curr_error - prev_error) / prev_error > cfg.jac_update_err_inc_threshold)
      return want(kLinearize, guess, guess_scale);
    update_jac = false;
    return after_linearize();
  }
  Ask after_linearize()
  {
    // TrackFrame without the match-geometry term: "no overlap" ends the tracking with a failure (:1515-1519)
    if (cfg.no_overlap_error > 0.f && curr_error >= cfg.no_overlap_error)
      return done(SAGE_E_NO_OVERLAP);
    curr_iter += 1;
    const int rc = sage_damped_solve_qr_f32(AtA, Atb, dof, damp, sol);
    if (rc != 0)
      return done(rc, true);
    if (lm_converged(cfg, dof, guess, guess_scale, Atb, sol))
      return done(SAGE_OK);
    return propose();
  }
  Ask propose()
  {
    sage_pose_retract(guess, sol, cand); // UpdateVariables (:467-512)
    cand_scale = dof == 7 ? guess_scale + sol[6] : guess_scale;
    return want(kError, cand, cand_scale);
  }
  Ask after_inner(bool accepted)
  {
    if (trace && ntrace < trace_cap)
      trace[ntrace++] = SageLmTraceEntry{damp, curr_error, cand_error, accepted ? 1 : 0, update_jac ? 1 : 0};
    if (cand_error >= curr_error && damp >= cfg.max_damp)
      return done(SAGE_OK);
    std::memcpy(guess, cand, sizeof(guess));
    guess_scale = cand_scale;
    if (update_jac)
      prev_error = curr_error;
    curr_error = cand_error;
    damp = clampd(damp / cfg.damp_dec_factor);
    if (curr_iter >= cfg.max_num_iters)
      return done(SAGE_OK);
    return top();
  }

public:
  void results(float *pose12, float *scale, float *final_error, int *iters, int *trace_len) const
  {
    std::memcpy(pose12, guess, sizeof(guess));
    if (scale)
      *scale = guess_scale;
    if (final_error)
      *final_error = curr_error;
    if (iters)
      *iters = (int)curr_iter;
    if (trace_len)
      *trace_len = ntrace;
  }
};

} // namespace sage

extern "C" int sage_track_lm(const SageLmConfig *cfgp, int dof, SageTrackLinearizeFn lin, SageTrackErrorFn errf,
                             void *ctx, float *pose12, float *scale, float *final_error, int *iters,
                             SageLmTraceEntry *trace, int trace_cap, int *trace_len)
{
  if (!cfgp || !lin || !errf || !pose12 || (dof != 6 && dof != 7) || (dof == 7 && !scale))
    return SAGE_E_INVALID;
  sage::LmStepper st;
  st.init(*cfgp, dof, pose12, scale, trace, trace_cap);
  sage::LmStepper::Ask ask = st.start();
  while (ask != sage::LmStepper::kDone)
  {
    float e = ask == sage::LmStepper::kLinearize ? 0.f : st.cand_error;
    const int rc = ask == sage::LmStepper::kLinearize ? lin(ctx, st.req_pose, st.req_scale, st.AtA, st.Atb, &e)
                                                      : errf(ctx, st.req_pose, st.req_scale, &e);
    if (rc != 0)
      return rc;
    ask = st.feed(st.AtA, st.Atb, e);
  }
  if (st.failed)
    return st.status;
  st.results(pose12, scale, final_error, iters, trace_len);
  return st.status;
}

extern "C" int sage_track_lm_batch(const SageLmConfig *cfgp, int dof, int B, SageTrackBatchEvalFn eval, void *ctx,
                                   float *pose12, float *scale, float *final_error, int *iters, int *status,
                                   SageLmTraceEntry *trace, int trace_cap, int *trace_len)
{
  if (!cfgp || !eval || !pose12 || !status || (dof != 6 && dof != 7) || (dof == 7 && !scale) || B < 0 ||
      B > SAGE_TRACK_MAX_BATCH)
    return SAGE_E_INVALID;
  if (B == 0)
    return SAGE_OK;
  using Ask = sage::LmStepper::Ask;
  std::vector<sage::LmStepper> st((size_t)B);
  for (int b = 0; b < B; ++b)
  {
    st[b].init(*cfgp, dof, pose12 + 12 * (size_t)b, scale ? scale + b : nullptr,
               trace ? trace + (size_t)b * (trace_cap > 0 ? trace_cap : 0) : nullptr, trace_cap);
    st[b].start();
  }
  // one round: every problem that is not done asks for exactly one evaluation, in ascending problem order
  int32_t problem[SAGE_TRACK_MAX_BATCH], want_jac[SAGE_TRACK_MAX_BATCH];
  std::vector<float> rp((size_t)B * 12), rs((size_t)B), A((size_t)B * 49), g((size_t)B * 7), e((size_t)B);
  while (true)
  {
    int n = 0;
    for (int b = 0; b < B; ++b)
    {
      if (st[b].ask == Ask::kDone)
      {
        if (st[b].failed)
          return st[b].status;
        continue;
      }
      problem[n] = b;
      want_jac[n] = st[b].ask == Ask::kLinearize ? 1 : 0;
      std::memcpy(&rp[(size_t)n * 12], st[b].req_pose, 12 * sizeof(float));
      rs[n] = st[b].req_scale;
      e[n] = want_jac[n] ? 0.f : st[b].cand_error;
      ++n;
    }
    if (n == 0)
      break;
    const int rc = eval(ctx, n, problem, want_jac, rp.data(), rs.data(), A.data(), g.data(), e.data());
    if (rc != 0)
      return rc;
    for (int i = 0; i < n; ++i)
      st[problem[i]].feed(&A[(size_t)i * 49], &g[(size_t)i * 7], e[i]);
  }
  for (int b = 0; b < B; ++b)
  {
    st[b].results(pose12 + 12 * (size_t)b, scale ? scale + b : nullptr, final_error ? final_error + b : nullptr,
                  iters ? iters + b : nullptr, trace_len ? trace_len + b : nullptr);
    status[b] = st[b].status;
  }
  return SAGE_OK;
}
