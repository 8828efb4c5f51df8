// registration_math.h -- the 3x3 mathematics of the registration's finish, one source for both sides: the host finish
// (registration_host.cpp, plain C++) and the device finish (reg_finish_kernel in registration.hip, __host__ __device__ under
// hipcc).  svdRot (utils.h:121-136) behind its nine sums: the 3x3 SVD as a one-sided Jacobi, the determinant fix, V U^T.
// Floating-point contraction is off in every function here: both sides round every product on its own, and a host and a
// device evaluation of the finish differ only in the order of their sums.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define SAGE_REG_HD __host__ __device__
#else
#define SAGE_REG_HD
#endif
#if defined(__clang__)
#define SAGE_REG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SAGE_REG_NO_CONTRACT // (g++ contracts only where the target has a fused multiply-add: build with -ffp-contract=off there)
#endif

namespace sage_reg
{
struct Mat3
{
  double m[3][3];
};

SAGE_REG_HD inline void cross3(const double *a, const double *b, double *c)
{
  SAGE_REG_NO_CONTRACT
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

SAGE_REG_HD inline double det3(const Mat3 &A)
{
  SAGE_REG_NO_CONTRACT
  return A.m[0][0] * (A.m[1][1] * A.m[2][2] - A.m[1][2] * A.m[2][1]) - A.m[0][1] * (A.m[1][0] * A.m[2][2] - A.m[1][2] * A.m[2][0]) +
         A.m[0][2] * (A.m[1][0] * A.m[2][1] - A.m[1][1] * A.m[2][0]);
}

// H = U S V^T by one-sided Jacobi on the columns of A = H (A V' = U S): columns ordered by descending norm; U's columns of a
// vanishing singular value are completed to a right-handed frame (det U = +1 whenever a column is completed).  At most 60
// sweeps
SAGE_REG_HD inline void svd3(const Mat3 &H, Mat3 &U, Mat3 &V)
{
  SAGE_REG_NO_CONTRACT
  double A[3][3], Vm[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      A[r][c] = H.m[r][c];
  for (int sweep = 0; sweep < 60; ++sweep)
  {
    double off = 0.0;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q)
      {
        double alpha = 0, beta = 0, gamma = 0;
        for (int r = 0; r < 3; ++r)
        {
          alpha += A[r][p] * A[r][p];
          beta += A[r][q] * A[r][q];
          gamma += A[r][p] * A[r][q];
        }
        if (gamma == 0.0 || fabs(gamma) <= 1e-300)
          continue;
        const double rel = fabs(gamma) / sqrt(alpha * beta);
        off = off < rel ? rel : off; // (std::max(off, rel): a NaN leaves off as it is)
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 3; ++r)
        {
          const double ap = A[r][p], aq = A[r][q];
          A[r][p] = c * ap - s * aq;
          A[r][q] = s * ap + c * aq;
          const double vp = Vm[r][p], vq = Vm[r][q];
          Vm[r][p] = c * vp - s * vq;
          Vm[r][q] = s * vp + c * vq;
        }
      }
    if (!(off > 1e-16)) // (also leaves on a NaN)
      break;
  }
  double sv[3];
  for (int c = 0; c < 3; ++c)
    sv[c] = sqrt(A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c]);
  // the columns by descending norm, equal norms in their own order: an insertion sort of three entries, which moves an
  // entry only past a strictly smaller one (the order a stable sort by sv[a] > sv[b] gives)
  int order[3] = {0, 1, 2};
  for (int i = 1; i < 3; ++i)
  {
    const int o = order[i];
    int k = i;
    for (; k > 0 && sv[o] > sv[order[k - 1]]; --k)
      order[k] = order[k - 1];
    order[k] = o;
  }
  double u[3][3]; // u[k]: the k-th left vector
  const double tiny = sv[order[0]] * 1e-13;
  int rank = 0;
  for (int k = 0; k < 3; ++k)
  {
    const int c = order[k];
    for (int r = 0; r < 3; ++r)
      V.m[r][k] = Vm[r][c];
    if (sv[c] > tiny && sv[c] > 0.0 && rank == k)
    {
      for (int r = 0; r < 3; ++r)
        u[k][r] = A[r][c] / sv[c];
      rank = k + 1;
    }
  }
  if (rank == 0)
  {
    u[0][0] = 1; u[0][1] = 0; u[0][2] = 0;
    u[1][0] = 0; u[1][1] = 1; u[1][2] = 0;
  }
  else if (rank == 1)
  {
    // any unit vector perpendicular to u[0]: Gram-Schmidt on the axis u[0] is least aligned with
    int ax = 0;
    for (int r = 1; r < 3; ++r)
      if (fabs(u[0][r]) < fabs(u[0][ax]))
        ax = r;
    double e[3] = {0, 0, 0};
    e[ax] = 1.0;
    const double d = u[0][ax];
    double n = 0;
    for (int r = 0; r < 3; ++r)
    {
      u[1][r] = e[r] - d * u[0][r];
      n += u[1][r] * u[1][r];
    }
    n = sqrt(n);
    for (int r = 0; r < 3; ++r)
      u[1][r] /= n;
  }
  if (rank < 3)
    cross3(u[0], u[1], u[2]);
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r)
      U.m[r][k] = u[k][r];
}

// utils.h:121-136 behind H = X diag(W) Y^T: R = V U^T with V's last column negated when det U det V < 0
SAGE_REG_HD inline Mat3 svd_rot_of(const Mat3 &H)
{
  SAGE_REG_NO_CONTRACT
  Mat3 U, V;
  svd3(H, U, V);
  if (det3(U) * det3(V) < 0)
    for (int r = 0; r < 3; ++r)
      V.m[r][2] = -V.m[r][2];
  Mat3 R;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      R.m[r][c] = V.m[r][0] * U.m[c][0] + V.m[r][1] * U.m[c][1] + V.m[r][2] * U.m[c][2];
  return R;
}
} // namespace sage_reg
