// block_solver.h -- the host block solver (block_solver.cpp): fixed-block Cholesky of a window's normal equations on the
// storage the device scatter kernel produces, and the elimination-order planner that lays that storage out.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>

#include "host_threads.h" // the threads the block solve runs on, block_chol_arm, SolveLease

namespace sage
{
// Padded block size of the fixed-block Cholesky for B unknowns per keyframe: the B x B blocks are padded with identity
// rows to 8, 24 or 40 (8: the pose-scale systems of windows that hold every code, window_plan.h: solver_rows).  0: B
// outside 1..40, no block kernel for it.
inline int padded_block(int B) { return B < 1 ? 0 : B <= 8 ? 8 : B <= 24 ? 24 : B <= 40 ? 40 : 0; }

// Block-envelope Cholesky solve on the storage the device scatter kernel produces (solve_kernels.hip).  Row i keeps
// the blocks of columns B = [row_first[i], i] at T + (row_off[i] + j - row_first[i]) * Bp*Bp and, optionally, a
// second range A = [a_first[i], a_first[i] + a_cnt[i]) (all < row_first[i]) at T + (a_off[i] + j - a_first[i]) * Bp*Bp;
// columns between the two ranges are structurally zero in the factor.  Every block holds the TRANSPOSED block
// ([c][r] = A[i*Bp + r][j*Bp + c]); Bp is 40, 24 or 8.
// n1/n2 > 0 declare that rows [0,n1) and [n1,n1+n2) do not reference each other (two halves of a window split at a
// separator, solve_kernels.hip solver_create): they are factorised concurrently on two cores when a helper thread is
// armed (block_chol_arm, host_threads.h), otherwise one after the other.
struct BlockEnvelope
{
  int K = 0, Bp = 0;
  const int32_t *row_first = nullptr, *row_off = nullptr;
  const int32_t *a_first = nullptr, *a_cnt = nullptr, *a_off = nullptr; // may be null: no A ranges
  int n1 = 0, n2 = 0;
  // optional: ready[b] == epoch once block b of the storage (and, for a diagonal block, its rows of y) has been
  // delivered by the device; a row is only touched after all its blocks have arrived
  const volatile unsigned *ready = nullptr;
  unsigned epoch = 0;
  // optional, only ever set together with `ready` (solver_run), so `fill` alone is the test: fill[b] != 0 marks a block
  // that is structural fill-in (no link behind it, off the diagonal): the device does not deliver it -- whoever touches it
  // first zeroes it instead of waiting for a ticket (r05: the arrow rows of a loop-closure plan are ~1500 such blocks,
  // 19 MB of zeros that used to cross PCIe behind everything else while the arrow-row tasks waited for them)
  const uint8_t *fill = nullptr;
  // set from block_chol_arm's return value: the halves run WITHOUT their look-ahead stages, whose two cores carry arrow-row
  // chains instead (loop-closure plans with more long chains than the halves' L3 domain has cores left: r05)
  bool no_lookahead = false;
  // optional (set by block_chol_solve_tr): progress[h] = 1 + the last factorised row of half h (0: rows [0, n1),
  // 1: rows [n1, n1 + n2)), published after the row's forward substitution -- the arrow-row tasks follow it
  std::atomic<int> *progress = nullptr;
  // optional: for every column j the rows i > j that store a block (i, j), ascending (col_rows[col_ptr[j] .. col_ptr[j+1]));
  // the back substitution then visits exactly those instead of scanning all rows below j
  const int32_t *col_ptr = nullptr, *col_rows = nullptr;
  // back substitution: rows m >= bs_skip_from are left out of  sum_m L_mi^T x_m  (their part has been subtracted from y
  // beforehand, in parallel: the arrow rows of a loop-closure plan)
  int bs_skip_from = 0x7fffffff;
  // optional (set by block_chol_solve_tr): two threads per half.  pipe[h] = {rows of half h whose EARLY part is done,
  // rows that are complete}: a look-ahead thread forms, for row i, everything that only needs the rows <= i-2 (all
  // blocks but (i, i-1) and their share of (i, i-1) / the diagonal), the half's own thread follows with the chain that
  // needs row i-1 -- same blocks, same order of the sums, so the factor is the same bit for bit.
  struct RowPipe
  {
    alignas(64) std::atomic<int> early{0};
    alignas(64) std::atomic<int> late{0};
    // r05: the separator rows' blocks against this half's columns, formed by the half's look-ahead thread right behind the
    // rows they depend on (sep_pre): 0 nobody does it (the separator pass forms them itself), 1 pending, 2 done, -1 given up
    alignas(64) std::atomic<int> pre{0};
  };
  RowPipe *pipe = nullptr;
  bool sep_pre = false; // plain split windows: the look-ahead threads pre-form the separator rows' half blocks

  // ---- the storage view: the one place that knows where a block lives
  struct Range
  {
    int lo, hi; // columns [lo, hi)
  };
  Range a_range(int i) const
  {
    const int a = a_cnt ? a_first[i] : 0;
    return {a, a + (a_cnt ? a_cnt[i] : 0)};
  }
  Range b_range(int i) const { return {row_first[i], i}; } // (without the diagonal block (i, i))
  bool has(int i, int j) const
  {
    const Range a = a_range(i);
    return (j >= row_first[i] && j <= i) || (j >= a.lo && j < a.hi);
  }
  // storage index of block (i, j); (i, j) must be stored.  An envelope without A ranges never has j < row_first[i].
  size_t index(int i, int j) const
  {
    return (size_t)(j < row_first[i] ? a_off[i] + j - a_first[i] : row_off[i] + j - row_first[i]);
  }
  double *block(double *T, int i, int j) const { return T + index(i, j) * (size_t)(Bp * Bp); }
  // the columns of half `half` (0: rows [0, n1), 1: rows [n1, n1 + n2)) that separator row `srow` stores
  Range sep_range(int srow, int half) const
  {
    if (half == 0)
      return a_range(srow);
    const int sep0 = n1 + n2;
    return {std::min((int)row_first[srow], sep0), sep0};
  }
};
// In place: T becomes L^T blockwise, X (K*Bp*Bp) receives the inverses of the diagonal factors, y (K*Bp) the
// right-hand side on entry and the solution on return.  Returns 0, or 1 + the block column of the first non-positive
// pivot, -1 for an unsupported Bp, -2 when a block's ticket did not arrive within two seconds.  A split plan (n1 > 0)
// hands work to whichever helper / pool is armed, also by another caller: call it under a SolveLease (host_threads.h).
int block_chol_solve_tr(const BlockEnvelope &env, double *T, double *X, double *y);
// Partial factorisation for domain decomposition (shard_solve.cpp; storage as above, no A ranges): rows [0, nI) are
// factorised and forward-substituted; the separator rows [nI, K) receive L_ij for j < nI, their blocks (i, j >= nI) end
// as the Schur complement C_ij^T = (A_ij - sum_{k<nI} L_ik L_jk^T)^T and y_i as c_i = b_i - sum_{k<nI} L_ik y_k.
// block_chol_partial_back: x of the rows [0, nI) given x of the separators in y[nI..K).  Returns as block_chol_solve_tr.
int block_chol_partial(const BlockEnvelope &env, double *T, double *X, double *y, int nI);
int block_chol_partial_back(const BlockEnvelope &env, double *T, double *X, double *y, int nI);
int block_plan_long_arrow_chains(const BlockEnvelope &env);
// true when the separator rows of the plan reach far into the halves (cover keyframes of loop closures): the
// factorisation then wants the worker pool
bool block_plan_has_arrow_rows(const BlockEnvelope &env);

// Elimination order and block storage plan of a window's normal equations (K keyframe blocks, links (a,b), a < b).
// perm[position] = keyframe, pos[keyframe] = position.  Block b of the storage is (blk_row[b], blk_col[b]) in
// positions; blk_src[b] = link index, | 0x40000000 when the stored (transposed) block is the packed link block read
// row-major (row keyframe == a), or -1 for diagonal / fill-in blocks.
struct BlockPlan
{
  std::vector<int32_t> perm, pos, row_first, row_off, a_first, a_cnt, a_off, blk_row, blk_col, blk_src;
  std::vector<int32_t> col_ptr, col_rows; // BlockEnvelope::col_ptr / col_rows
  int nblk = 0, n1 = 0, n2 = 0;
  int index(int i, int j) const // storage index of block (i, j), as BlockEnvelope::index
  {
    return j < row_first[i] ? a_off[i] + j - a_first[i] : row_off[i] + j - row_first[i];
  }
};
int plan_blocks(int K, const std::vector<std::pair<int, int>> &links, bool may_split, BlockPlan &out);
// the envelope of a plan's storage with Bp-padded blocks: K, Bp, the five range tables, n1 / n2 and the column lists.
// The caller adds what is its own (ready / epoch / fill / no_lookahead); the plan must outlive the envelope.
BlockEnvelope envelope_of(const BlockPlan &plan, int Bp);
// What sage_block_solve factorises, for whoever else wants that factor (covariance_host.cpp): the plan of `links` (duplicates
// summed), the damped system (H + diag_add) + damp diag(H + diag_add) of a packed buffer scattered into the plan's storage T
// at padded_block(B), and the right-hand side g + g_add in y.  SAGE_OK, or what plan_blocks / padded_block refuse.
int block_system_build(const double *packed, int K, int nlinks, const int32_t *links, int B, double damp, const double *diag_add,
                       const double *g_add, BlockPlan &bp, std::vector<double> &T, std::vector<double> &y);
// ... and its factorisation under a SolveLease with the helpers armed as the plan wants them: block_chol_solve_tr's return
int block_system_factor(const BlockPlan &bp, int Bp, double *T, double *X, double *y);
} // namespace sage
