// covariance.h -- marginal covariances from the block Cholesky factor a solve leaves behind (covariance_host.cpp): the
// selected inverse of the block-envelope factor, i.e. the blocks of Sigma = M^-1 on the factor's own pattern, by one backward
// recursion over M = L L^T and no second factorisation.  Standard library only -- no HIP, no environment.
//
// Convention: positions j = K-1 .. 0 of the elimination order, col(j) = the rows below j that store a block of column j,
//   Sigma_ij = -(sum_{k in col(j)} Sigma_ik L_kj) L_jj^-1                      for every kept i > j (Sigma_ik = Sigma_ki^T, k > i)
//   Sigma_jj = (L_jj^-T - sum_{k in col(j)} Sigma_jk L_kj) L_jj^-1              then symmetrised exactly, (S + S^T) / 2.
// The recursion reads Sigma_ik for every pair i, k of col(j): the kept pattern must be CLOSED under "two rows of one column
// are a block".  A plain envelope is closed (blocks (i, j), (k, j), j < k < i: k >= row_first[i]); for plans with A ranges
// (separator rows, the arrow rows of cover keyframes) CovPlan does not assume it: it is the symbolic closure of the stored
// pattern, computed once per BlockPlan.  Blocks the closure adds are working storage: their L is structurally zero.
#pragma once

#include <stdint.h>

#include <vector>

#include "block_solver.h"

namespace sage
{
namespace cov
{

struct CovPlan
{
  int K = 0, nblk = 0, added = 0;          // Sigma blocks kept (lower triangle, diagonal included); of them added by the closure
  std::vector<int32_t> col_ptr, col_rows;  // per column j the rows i > j that keep Sigma_ij, ascending (the closed pattern)
  std::vector<int32_t> index;              // [K * K]: Sigma block of (i, j), i >= j, or -1
  int at(int i, int j) const { return i >= j ? index[(size_t)i * K + j] : index[(size_t)j * K + i]; }
};
CovPlan plan_covariance(const BlockPlan &plan);

// The recursion, on the calling thread, in one fixed order.  T / X: what block_chol_solve_tr left (blockwise L^T and the
// inverses of the diagonal factors, Bp-padded: 8, 24 or 40).  Sigma [cp.nblk][Bp * Bp] row-major, block (i, j) = rows of
// position i, columns of position j, padded like the factor: the identity padding rows stay apart from the others and are
// skipped on the way out.
void selected_inverse(const BlockPlan &plan, const CovPlan &cp, int Bp, const double *T, const double *X, double *Sigma);

// the Bs x Bs head of block (pa, pb) of Sigma in positions, either order, row-major into out [Bs * Bs]: the stored block or its
// transpose, bit for bit.  false: the pair keeps no block
bool covariance_block(const CovPlan &cp, int Bp, int Bs, const double *Sigma, int pa, int pb, double *out);

} // namespace cov
} // namespace sage
