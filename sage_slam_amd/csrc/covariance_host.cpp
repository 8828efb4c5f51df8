// covariance_host.cpp -- the host side of the marginal covariances (covariance.h): the symbolic closure of a plan's pattern,
// the backward recursion over the factor, and the stateless entry point next to sage_block_solve.  Plain C++17, no HIP include.
// The recursion runs where the factor lies: it is one more dependency chain over the K block columns (about as many
// multiply-adds as the factorisation's own), and the factor is in host memory after every solve.
#include "covariance.h"

#include <algorithm>
#include <cstring>

#include "host_math.h" // env_flag
#include "sage_ba.h"

namespace sage
{
namespace cov
{

CovPlan plan_covariance(const BlockPlan &plan)
{
  CovPlan cp;
  const int K = (int)plan.row_first.size();
  cp.K = K;
  std::vector<std::vector<int32_t>> rows(K);
  std::vector<char> has((size_t)K * K, 0);
  int stored = K;
  for (int j = 0; j < K; ++j)
    for (int q = plan.col_ptr[j]; q < plan.col_ptr[j + 1]; ++q)
    {
      rows[j].push_back(plan.col_rows[q]);
      has[(size_t)plan.col_rows[q] * K + j] = 1;
      ++stored;
    }
  // columns ascending: a pair k < i of column j is a block (i, k) of a LATER column, whose own pairs are formed when its turn
  // comes (symbolic elimination)
  for (int j = 0; j < K; ++j)
  {
    std::sort(rows[j].begin(), rows[j].end());
    for (size_t a = 0; a < rows[j].size(); ++a)
      for (size_t b = a + 1; b < rows[j].size(); ++b)
      {
        const int k = rows[j][a], i = rows[j][b];
        if (!has[(size_t)i * K + k])
        {
          has[(size_t)i * K + k] = 1;
          rows[k].push_back(i);
        }
      }
  }
  cp.index.assign((size_t)K * K, -1);
  cp.col_ptr.assign(K + 1, 0);
  int n = 0;
  for (int j = 0; j < K; ++j)
  {
    cp.index[(size_t)j * K + j] = n++;
    for (int i : rows[j])
    {
      cp.index[(size_t)i * K + j] = n++;
      cp.col_rows.push_back(i);
    }
    cp.col_ptr[j + 1] = (int32_t)cp.col_rows.size();
  }
  cp.nblk = n;
  cp.added = n - stored;
  return cp;
}

namespace
{
// C [N x N] += A B (ta: A^T B), all row-major: one scalar of A against a contiguous row of B, rows and columns ascending.
// N is a padded block size: whole vectors, compile-time trip counts
template <int N>
static inline __attribute__((always_inline)) void gemm_fixed(double *C, const double *A, bool ta, const double *Bm)
{
  for (int r = 0; r < N; ++r)
  {
    double c[N];
    for (int col = 0; col < N; ++col)
      c[col] = C[r * N + col];
    for (int t = 0; t < N; ++t)
    {
      const double a = ta ? A[t * N + r] : A[r * N + t];
      const double *b = Bm + t * N;
      for (int col = 0; col < N; ++col)
        c[col] += a * b[col];
    }
    for (int col = 0; col < N; ++col)
      C[r * N + col] = c[col];
  }
}
// (one clone per vector width, as the block solver's kernels: the order of the sums is the same in each)
__attribute__((target_clones("avx512f", "avx2", "default"))) void gemm_acc(double *C, const double *A, bool ta, const double *Bm, int n)
{
  if (n == 40)
    gemm_fixed<40>(C, A, ta, Bm);
  else if (n == 24)
    gemm_fixed<24>(C, A, ta, Bm);
  else
    gemm_fixed<8>(C, A, ta, Bm);
}
// a transposed block as the plain matrix: out[r][c] = Tb[c * n + r]
void untranspose(double *out, const double *Tb, int n)
{
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c)
      out[(size_t)r * n + c] = Tb[(size_t)c * n + r];
}
} // namespace

void selected_inverse(const BlockPlan &plan, const CovPlan &cp, int Bp, const double *T, const double *X, double *Sigma)
{
  // on the padded blocks as they lie: the padding rows are a multiple of the identity in L_jj and zero in every L_kj, so
  // they stay apart from the others in every product below -- and the micro-kernel gets whole vectors
  const int K = cp.K, n = Bp;
  const size_t nn = (size_t)n * n, BBp = nn;
  int widest = 0;
  for (int j = 0; j < K; ++j)
    widest = std::max(widest, (int)(plan.col_ptr[j + 1] - plan.col_ptr[j]));
  std::vector<double> Lcol((size_t)widest * nn), Linv(nn), W(nn), D(nn);
  for (int j = K - 1; j >= 0; --j)
  {
    const int32_t *lrows = plan.col_rows.data() + plan.col_ptr[j];
    const int nl = plan.col_ptr[j + 1] - plan.col_ptr[j];
    for (int q = 0; q < nl; ++q) // L_kj: the stored block is its transpose
      untranspose(&Lcol[q * nn], T + (size_t)plan.index(lrows[q], j) * BBp, n);
    untranspose(Linv.data(), X + (size_t)j * BBp, n); // X = L_jj^-T
    for (int qi = cp.col_ptr[j]; qi < cp.col_ptr[j + 1]; ++qi)
    {
      const int i = cp.col_rows[qi];
      std::fill(W.begin(), W.end(), 0.0);
      for (int q = 0; q < nl; ++q)
      {
        const int k = lrows[q];
        gemm_acc(W.data(), Sigma + (size_t)cp.at(i, k) * nn, k > i, &Lcol[q * nn], n);
      }
      for (double &v : W)
        v = -v;
      double *Sij = Sigma + (size_t)cp.at(i, j) * nn;
      std::fill(Sij, Sij + nn, 0.0);
      gemm_acc(Sij, W.data(), false, Linv.data(), n);
    }
    // the diagonal block: Sigma_jk = Sigma_kj^T, just formed
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c)
        W[(size_t)r * n + c] = Linv[(size_t)c * n + r]; // L_jj^-T
    std::fill(D.begin(), D.end(), 0.0);
    for (int q = 0; q < nl; ++q)
      gemm_acc(D.data(), Sigma + (size_t)cp.at(lrows[q], j) * nn, true, &Lcol[q * nn], n);
    for (size_t o = 0; o < nn; ++o)
      W[o] -= D[o];
    std::fill(D.begin(), D.end(), 0.0);
    gemm_acc(D.data(), W.data(), false, Linv.data(), n);
    double *Sjj = Sigma + (size_t)cp.at(j, j) * nn;
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c)
        Sjj[(size_t)r * n + c] = 0.5 * (D[(size_t)r * n + c] + D[(size_t)c * n + r]);
  }
}

bool covariance_block(const CovPlan &cp, int Bp, int Bs, const double *Sigma, int pa, int pb, double *out)
{
  const int b = cp.at(pa, pb);
  if (b < 0)
    return false;
  const double *S = Sigma + (size_t)b * Bp * Bp;
  for (int r = 0; r < Bs; ++r)
    for (int c = 0; c < Bs; ++c)
      out[(size_t)r * Bs + c] = pa >= pb ? S[(size_t)r * Bp + c] : S[(size_t)c * Bp + r];
  return true;
}

} // namespace cov
} // namespace sage

extern "C" int sage_block_covariance(const double *packed, int K, int nlinks, const int32_t *links, int B, double damp,
                                     const double *diag_add, const int32_t *pairs, int n_pairs, double *Sigma)
{
  if (!packed || K < 1 || B < 1 || nlinks < 0 || (nlinks > 0 && !links) || n_pairs < 0 || (n_pairs > 0 && (!pairs || !Sigma)))
    return SAGE_E_INVALID;
  const int Bp = sage::padded_block(B);
  sage::BlockPlan bp;
  std::vector<double> T, y;
  if (const int rcb = sage::block_system_build(packed, K, nlinks, links, B, damp, diag_add, nullptr, bp, T, y))
    return rcb;
  for (int p = 0; p < n_pairs; ++p) // a pair is a keyframe with itself or a link, either way round
  {
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    bool ok = a >= 0 && a < K && a == b;
    for (int l = 0; l < nlinks && !ok; ++l)
      ok = (links[2 * l] == a && links[2 * l + 1] == b) || (links[2 * l] == b && links[2 * l + 1] == a);
    if (!ok)
      return SAGE_E_INVALID;
  }
  std::vector<double> X((size_t)K * Bp * Bp);
  std::fill(y.begin(), y.end(), 0.0); // (the factor is all that is wanted: the substitutions run on zeros)
  if (sage::block_system_factor(bp, Bp, T.data(), X.data(), y.data()) != 0)
    return SAGE_E_NOT_PSD; // (nothing written)
  const sage::cov::CovPlan cp = sage::cov::plan_covariance(bp);
  std::vector<double> S((size_t)cp.nblk * Bp * Bp);
  sage::cov::selected_inverse(bp, cp, Bp, T.data(), X.data(), S.data());
  for (int p = 0; p < n_pairs; ++p)
    sage::cov::covariance_block(cp, Bp, B, S.data(), bp.pos[pairs[2 * p]], bp.pos[pairs[2 * p + 1]], Sigma + (size_t)p * B * B);
  return SAGE_OK;
}

// the closure as the tests see it: the blocks (lower triangle, diagonal included) the plan of K keyframes and `links` stores,
// and how many the closure adds to them
extern "C" int sage_covariance_plan(int K, int nlinks, const int32_t *links, int32_t *stored, int32_t *added)
{
  if (K < 1 || nlinks < 0 || (nlinks > 0 && !links))
    return SAGE_E_INVALID;
  std::vector<std::pair<int, int>> lk(nlinks);
  for (int l = 0; l < nlinks; ++l)
    lk[l] = {links[2 * l], links[2 * l + 1]};
  std::sort(lk.begin(), lk.end());
  lk.erase(std::unique(lk.begin(), lk.end()), lk.end());
  sage::BlockPlan bp;
  if (const int rc = sage::plan_blocks(K, lk, !sage::env_flag("SAGE_SOLVE_NO_SPLIT"), bp))
    return rc;
  const sage::cov::CovPlan cp = sage::cov::plan_covariance(bp);
  if (stored)
    *stored = cp.nblk - cp.added;
  if (added)
    *added = cp.added;
  return SAGE_OK;
}
