// block_solver.cpp -- the host block solver (block_solver.h): fixed-block Cholesky of the window's normal equations on
// host cores.  In order: the AVX-512 micro-kernels, the storage view, the ticket wait and the row primitives, the row
// passes (factor_rows / chain_rows / lookahead_rows / separator_prepass / back_substitute), the Schur rows of the sharded
// solve, the arrow-row tasks of loop-closure plans (SepJob, SepPool), the helper hand-shakes, the elimination-order
// planner (plan_blocks), the orchestration (block_chol_solve_tr) and sage_block_solve.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sched.h>
#include <thread>
#include <vector>

#include "block_solver.h"
#include "damped_system.h"
#include "host_math.h" // env_flag
#include "sage_ba.h"

// ------------------------------------------------------------------------------------------------
// Fixed-block-size Cholesky on transposed block storage (the window solve's host leg).
//
// Every finished block is kept as T_ij = L_ij^T (row t of T = column t of L), the diagonal factors as U = L^T and
// X = U^-1.  With that layout every contraction is "broadcast one scalar, multiply a contiguous row":
//   C_ij^T[c][:]  -= sum_k sum_t T_jk[t][c] * T_ik[t][:]         (trailing update)
//   T_ij[c][:]     = sum_{t<=c} X_j[t][c] * C_ij^T[t][:]          (L_ij = C_ij L_jj^-T)
// so the micro-kernel is 4 output rows x NV vectors of accumulators, NV loads + 4 broadcasts + 4*NV FMAs per step,
// no horizontal sums.
// ------------------------------------------------------------------------------------------------
namespace sage
{
namespace
{
typedef double v8d __attribute__((vector_size(64), aligned(8)));

// (macros, not functions: a v8d crossing a function boundary would need the AVX-512 ABI in every clone)
#define SAGE_LOADU(dst, p) __builtin_memcpy(&(dst), (p), sizeof(v8d))
#define SAGE_STOREU(p, v) __builtin_memcpy((p), &(v), sizeof(v8d))

// The blocks of a row arrive by DMA straight into DRAM (no cache allocation on this platform): a row's first touch of
// its ~4 fresh blocks (51 KB) would stall the core for ~2 us.  The contraction loops of row i therefore prefetch row
// i+1's blocks, two cache lines per inner step.
struct RowPrefetch // (plain aggregate: the multi-versioned callers must not need an out-of-line constructor)
{
  const char *p, *end;
  // two more ranges, taken up when the first is through (r05, arrow-row chains: besides the chain's own next block the
  // half's blocks and inverse of the NEXT column -- written by another core, 64 KB a chain used to wait for column by column)
  const char *p2 = nullptr, *end2 = nullptr, *p3 = nullptr, *end3 = nullptr;
  inline __attribute__((always_inline)) void step()
  {
    if (p < end)
    {
      __builtin_prefetch(p, 0, 3);
      __builtin_prefetch(p + 64, 0, 3);
      p += 128;
    }
    else if (p2 < end2)
    {
      __builtin_prefetch(p2, 0, 3);
      __builtin_prefetch(p2 + 64, 0, 3);
      p2 += 128;
    }
    else if (p3 < end3)
    {
      __builtin_prefetch(p3, 0, 3);
      __builtin_prefetch(p3 + 64, 0, 3);
      p3 += 128;
    }
  }
};

// CT[c][8*V0 ..] -= sum_t Tj[t][c] * Ti[t][8*V0 ..]  for the 4 rows c0..c0+3 ; vectors V0..NV-1 only
template <int NV, int V0>
static inline __attribute__((always_inline)) void tn_sub_rows4(double *CT, const double *Tj, const double *Ti, int c0,
                                                               RowPrefetch &pf)
{
  constexpr int BP = NV * 8;
  v8d acc[4][NV];
  for (int u = 0; u < 4; ++u)
    for (int v = V0; v < NV; ++v)
      acc[u][v] = v8d{0, 0, 0, 0, 0, 0, 0, 0};
  for (int t = 0; t < BP; ++t)
  {
    const double *ti = Ti + t * BP, *tj = Tj + t * BP + c0;
    pf.step();
    v8d b[NV];
    for (int v = V0; v < NV; ++v)
      SAGE_LOADU(b[v], ti + 8 * v);
    for (int u = 0; u < 4; ++u)
    {
      const double sc = tj[u];
      const v8d s = {sc, sc, sc, sc, sc, sc, sc, sc};
      for (int v = V0; v < NV; ++v)
        acc[u][v] += s * b[v];
    }
  }
  for (int u = 0; u < 4; ++u)
    for (int v = V0; v < NV; ++v)
    {
      v8d c;
      SAGE_LOADU(c, CT + (c0 + u) * BP + 8 * v);
      c -= acc[u][v];
      SAGE_STOREU(CT + (c0 + u) * BP + 8 * v, c);
    }
}

// CT -= Tj^T-contraction with Ti over the whole block; upper_only: only entries [c][r >= c] are needed (diagonal
// block, symmetric) -> the vectors left of the diagonal are skipped
template <int NV>
static inline __attribute__((always_inline)) void tn_sub(double *CT, const double *Tj, const double *Ti, bool upper_only,
                                                         RowPrefetch &pf)
{
  constexpr int BP = NV * 8;
  for (int c0 = 0; c0 < BP; c0 += 4)
  {
    const int v0 = upper_only ? c0 / 8 : 0;
    switch (v0)
    {
    case 0: tn_sub_rows4<NV, 0>(CT, Tj, Ti, c0, pf); break;
    case 1: tn_sub_rows4<NV, (NV > 1 ? 1 : 0)>(CT, Tj, Ti, c0, pf); break;
    case 2: tn_sub_rows4<NV, (NV > 2 ? 2 : 0)>(CT, Tj, Ti, c0, pf); break;
    case 3: tn_sub_rows4<NV, (NV > 3 ? 3 : 0)>(CT, Tj, Ti, c0, pf); break;
    default: tn_sub_rows4<NV, (NV > 4 ? 4 : 0)>(CT, Tj, Ti, c0, pf); break;
    }
  }
}

// in place: CT[c][:] <- sum_{t<=c} X[t][c] * CT[t][:]   (rows in descending groups of 4: a group reads rows <= its own)
template <int NV>
static inline __attribute__((always_inline)) void apply_inverse(double *CT, const double *X)
{
  constexpr int BP = NV * 8;
  for (int c0 = BP - 4; c0 >= 0; c0 -= 4)
  {
    v8d acc[4][NV];
    for (int u = 0; u < 4; ++u)
      for (int v = 0; v < NV; ++v)
        acc[u][v] = v8d{0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t <= c0 + 3; ++t)
    {
      const double *ct = CT + t * BP, *xs = X + t * BP + c0; // X[t][c] = 0 for c < t
      v8d b[NV];
      for (int v = 0; v < NV; ++v)
        SAGE_LOADU(b[v], ct + 8 * v);
      for (int u = 0; u < 4; ++u)
      {
        const double sc = xs[u];
        const v8d s = {sc, sc, sc, sc, sc, sc, sc, sc};
        for (int v = 0; v < NV; ++v)
          acc[u][v] += s * b[v];
      }
    }
    for (int u = 0; u < 4; ++u)
      for (int v = 0; v < NV; ++v)
        SAGE_STOREU(CT + (c0 + u) * BP + 8 * v, acc[u][v]);
  }
}

// One 8-row panel of the Cholesky factorisation below, everything with compile-time indices so that the panel's
// diagonal block lives in eight registers: the pivot chain (sqrt, divide, seven multiplier broadcasts) never goes
// through memory -- a scalar reload of a just-stored vector element does not forward and cost more than the sqrt.
template <int NV, int P>
static inline __attribute__((always_inline)) bool factor_panel(double *S, double *rinv)
{
  constexpr int BP = NV * 8;
  v8d D[8];
  for (int cc = 0; cc < 8; ++cc)
    SAGE_LOADU(D[cc], S + (8 * P + cc) * BP + 8 * P);
  double rsv[8];
#pragma unroll
  for (int cc = 0; cc < 8; ++cc)
  {
    const double d = D[cc][cc];
    if (!(d > 0.0))
      return false;
    const double rs = 1.0 / std::sqrt(d);
    rsv[cc] = rs;
    rinv[8 * P + cc] = rs; // 1 / U[c][c]
    const v8d rv = {rs, rs, rs, rs, rs, rs, rs, rs};
    D[cc] *= rv;
#pragma unroll
    for (int c2 = cc + 1; c2 < 8; ++c2)
    {
      const double f = D[cc][c2];
      const v8d fv = {f, f, f, f, f, f, f, f};
      D[c2] -= fv * D[cc];
    }
  }
  // U is upper triangular: clear what the updates left below the diagonal of the block, store the rows
#pragma unroll
  for (int cc = 0; cc < 8; ++cc)
  {
#pragma unroll
    for (int r = 0; r < cc; ++r)
      D[cc][r] = 0.0;
    SAGE_STOREU(S + (8 * P + cc) * BP + 8 * P, D[cc]);
  }
  // the same eliminations on the panel's other columns (independent of the pivot chain)
#pragma unroll
  for (int v = P + 1; v < NV; ++v)
  {
    v8d R[8];
    for (int cc = 0; cc < 8; ++cc)
      SAGE_LOADU(R[cc], S + (8 * P + cc) * BP + 8 * v);
#pragma unroll
    for (int cc = 0; cc < 8; ++cc)
    {
      const v8d rv = {rsv[cc], rsv[cc], rsv[cc], rsv[cc], rsv[cc], rsv[cc], rsv[cc], rsv[cc]};
      R[cc] *= rv;
#pragma unroll
      for (int c2 = cc + 1; c2 < 8; ++c2)
      {
        const double f = D[cc][c2];
        const v8d fv = {f, f, f, f, f, f, f, f};
        R[c2] -= fv * R[cc];
      }
    }
    for (int cc = 0; cc < 8; ++cc)
      SAGE_STOREU(S + (8 * P + cc) * BP + 8 * v, R[cc]);
  }
  // rank-8 update of the trailing rows
  for (int c2 = 8 * P + 8; c2 < BP; ++c2)
  {
    double *row2 = S + c2 * BP;
    v8d f[8];
    for (int t = 0; t < 8; ++t)
    {
      const double ft = S[(8 * P + t) * BP + c2];
      f[t] = v8d{ft, ft, ft, ft, ft, ft, ft, ft};
    }
    for (int v = c2 / 8; v < NV; ++v)
    {
      v8d acc;
      SAGE_LOADU(acc, row2 + 8 * v);
      for (int t = 0; t < 8; ++t)
      {
        v8d x;
        SAGE_LOADU(x, S + (8 * P + t) * BP + 8 * v);
        acc -= f[t] * x;
      }
      SAGE_STOREU(row2 + 8 * v, acc);
    }
  }
  if constexpr (P + 1 < NV)
    return factor_panel<NV, P + 1>(S, rinv);
  else
    return true;
}

// X = U^-1 by back substitution on rows: X[c][:] = (e_c - sum_{t>c} U[c][t] X[t][:]) / U[c][c].  X[t][:] is zero left
// of column t, so a block of eight t only touches the vectors from its own on -- with the block index a template
// parameter every vector loop has compile-time bounds (a run-time start index would move the accumulators from
// registers to the stack).  Two accumulator sets (even / odd t) keep enough independent FMA chains in flight.
template <int NV, int TB>
static inline __attribute__((always_inline)) void inverse_accumulate(const double *u, const double *X, v8d *a0, v8d *a1)
{
  constexpr int BP = NV * 8;
#pragma unroll
  for (int tt = 0; tt < 8; tt += 2)
  {
    const int t = 8 * TB + tt;
    const double f0 = u[t], f1 = u[t + 1];
    const v8d fv0 = {f0, f0, f0, f0, f0, f0, f0, f0}, fv1 = {f1, f1, f1, f1, f1, f1, f1, f1};
#pragma unroll
    for (int v = TB; v < NV; ++v)
    {
      v8d xa, xb;
      SAGE_LOADU(xa, X + t * BP + 8 * v);
      SAGE_LOADU(xb, X + (t + 1) * BP + 8 * v);
      a0[v] -= fv0 * xa;
      a1[v] -= fv1 * xb;
    }
  }
  if constexpr (TB + 1 < NV)
    inverse_accumulate<NV, TB + 1>(u, X, a0, a1);
}

template <int NV, int CB>
static inline __attribute__((always_inline)) void inverse_rows(const double *S, double *X, const double *rinv)
{
  constexpr int BP = NV * 8;
  for (int cc = 7; cc >= 0; --cc)
  {
    const int c = 8 * CB + cc;
    double e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    e[cc] = 1.0;
    v8d a0[NV], a1[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v)
      a0[v] = a1[v] = v8d{0, 0, 0, 0, 0, 0, 0, 0};
    SAGE_LOADU(a0[CB], e);
    const double *u = S + c * BP;
    for (int t = c + 1; t < 8 * CB + 8; ++t) // the rest of the row's own block
    {
      const double f = u[t];
      const v8d fv = {f, f, f, f, f, f, f, f};
#pragma unroll
      for (int v = CB; v < NV; ++v)
      {
        v8d x;
        SAGE_LOADU(x, X + t * BP + 8 * v);
        a0[v] -= fv * x;
      }
    }
    if constexpr (CB + 1 < NV)
      inverse_accumulate<NV, CB + 1>(u, X, a0, a1);
    const double inv = rinv[c];
    const v8d iv = {inv, inv, inv, inv, inv, inv, inv, inv};
#pragma unroll
    for (int v = 0; v < NV; ++v)
    {
      v8d r = (a0[v] + a1[v]) * iv; // (zero for v < CB)
      SAGE_STOREU(X + c * BP + 8 * v, r);
    }
  }
  if constexpr (CB > 0)
    inverse_rows<NV, CB - 1>(S, X, rinv);
}

// S (symmetric, entries [c][r >= c] valid) -> U = L^T in place (A = U^T U), X = U^-1 (upper triangular, zeros below).
// Blocked by panels of 8 rows (factor_panel), one rank-8 register-accumulated update per trailing row.
template <int NV>
static inline __attribute__((always_inline)) bool factor_diag(double *S, double *X)
{
  constexpr int BP = NV * 8;
  double rinv[BP];
  if (!factor_panel<NV, 0>(S, rinv))
    return false;
  inverse_rows<NV, NV - 1>(S, X, rinv);
  return true;
}

// ---- the storage of one solve: blk(i, j) = where block (i, j) lives (BlockEnvelope::index with the block size folded in)
template <int NV>
struct Blocks
{
  const BlockEnvelope &E;
  double *T;
  inline __attribute__((always_inline)) double *operator()(int i, int j) const { return T + E.index(i, j) * (size_t)(NV * 8 * NV * 8); }
};

// the blocks of row r as a prefetch range: they are contiguous in the storage, [A range | B range]
template <int NV>
static inline __attribute__((always_inline)) RowPrefetch row_prefetch(const BlockEnvelope &E, const double *T, int r)
{
  constexpr size_t BB = (size_t)NV * 8 * NV * 8;
  const BlockEnvelope::Range a = E.a_range(r);
  const size_t b0 = (size_t)(a.hi > a.lo ? E.a_off[r] : E.row_off[r]);
  const size_t nb = (size_t)(a.hi - a.lo) + (size_t)(r - E.row_first[r] + 1);
  const char *p = reinterpret_cast<const char *>(T + b0 * BB);
  return RowPrefetch{p, p + nb * BB * sizeof(double)};
}

// ---- the ticket wait.  Block idx of the storage at its first touch: a structural fill block (E.fill) is zeroed, nobody
// delivers it; any other is spun on until it carries this solve's ticket (E.ready; no tickets: nothing to wait for).
// false: the ticket did not arrive within two seconds, or `abort` (optional: the arrow-row tasks' flag) was raised -- the
// flag is then set to 2 for the other tasks.  peek: read the ticket once before the clock (a whole row of delivered blocks
// costs no clock reads).
static inline __attribute__((always_inline)) bool wait_block(const BlockEnvelope &E, double *T, size_t idx,
                                                             std::atomic<int> *abort = nullptr, bool peek = false)
{
  const size_t BB = (size_t)E.Bp * E.Bp;
  if (E.fill && E.fill[idx])
  {
    std::memset(T + idx * BB, 0, BB * sizeof(double));
    return true;
  }
  if (!E.ready)
    return true;
  const volatile unsigned *f = E.ready + idx;
  if (!peek || *f != E.epoch)
  {
    const double t0 = mono_seconds();
    unsigned spins = 0;
    while (*f != E.epoch)
    {
      __builtin_ia32_pause();
      if ((++spins & 0xfff) == 0 && ((abort && abort->load(std::memory_order_acquire)) || mono_seconds() - t0 > 2.0))
      {
        if (abort)
          abort->store(2, std::memory_order_release);
        return false;
      }
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return true;
}

// The device streams the blocks in row order (solve_kernels.hip): wait until every block of row i carries this solve's
// ticket.  Only called with tickets (E.ready).
// from_col: only the blocks (i, j >= from_col) -- the others have been consumed already (the arrow-row tasks take their
// blocks one by one).  [skip_lo, skip_hi): blocks the separator pre-pass has taken care of, tickets and fill included.
static __attribute__((noinline)) bool wait_row_tickets(const BlockEnvelope &E, int i, double *T, int from_col = 0,
                                                       int skip_lo = 0, int skip_hi = 0)
{
  const BlockEnvelope::Range rg[2] = {E.a_range(i), {E.row_first[i], i + 1}};
  for (int r = 0; r < 2; ++r)
    for (int j = rg[r].lo; j < rg[r].hi; ++j)
      if (j >= from_col && !(j >= skip_lo && j < skip_hi) && !wait_block(E, T, E.index(i, j), nullptr, true))
        return false;
  return true;
}

// ---- row primitives (loop order and association are part of the result: bit-identical factor on every path)
#define SAGE_HSUM8(a) ((((a)[0] + (a)[4]) + ((a)[1] + (a)[5])) + (((a)[2] + (a)[6]) + ((a)[3] + (a)[7])))

// forward substitution with one block: w -= y_k (x) T_ik, i.e. w[r] -= sum_t yk[t] * Tk[t][r]
template <int NV>
static inline __attribute__((always_inline)) void fwd_sub_block(double *w, const double *Tk, const double *yk)
{
  constexpr int BP = NV * 8;
  for (int t = 0; t < BP; ++t)
  {
    const double f = yk[t];
    for (int r = 0; r < BP; ++r)
      w[r] -= f * Tk[t * BP + r];
  }
}

// y_i = w . X_i, i.e. y_i[c] = sum_t w[t] * X_i[t][c]  (X[t][c] = 0 for c < t)
template <int NV>
static inline __attribute__((always_inline)) void apply_diag_inverse(double *y_i, const double *w, const double *Xi)
{
  constexpr int BP = NV * 8;
  double yi[BP];
  for (int c = 0; c < BP; ++c)
    yi[c] = 0.0;
  for (int t = 0; t < BP; ++t)
  {
    const double f = w[t];
    for (int c = 0; c < BP; ++c)
      yi[c] += f * Xi[t * BP + c];
  }
  for (int c = 0; c < BP; ++c)
    y_i[c] = yi[c];
}

// back substitution of column i:  z[t] -= sum over the rows m below that store a block (m, i) of  sum_r T_mi[t][r] x_m[r].
// The rows: rows[0 .. nrows) ascending (a column list), or, rows == nullptr, every row i+1+q, q < nrows, that stores the
// block; the list ends at the first m >= skip_from.  8 values of t at a time keep one accumulator vector each across ALL
// those blocks (one horizontal sum per t and row instead of one per block -- the arrow rows of a loop-closure plan put
// half a dozen blocks into every column).
// (explicit vectors: strict fp semantics keep the compiler from vectorising a dot product on its own, and the scalar
// loops made this sweep a tenth of the solve)
template <int NV>
static inline __attribute__((always_inline)) void backsub_columns(double *z, Blocks<NV> blk, const double *y, int i,
                                                                  const int32_t *rows, int nrows, int skip_from)
{
  constexpr int BP = NV * 8;
  for (int t0 = 0; t0 < BP; t0 += 8)
  {
    v8d acc[8];
    for (int u = 0; u < 8; ++u)
      acc[u] = v8d{0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = 0; q < nrows; ++q)
    {
      const int m = rows ? rows[q] : i + 1 + q;
      if (m >= skip_from)
        break; // (ascending lists: the separator rows come last)
      if (!rows && !blk.E.has(m, i))
        continue;
      const double *Tm = blk(m, i) + t0 * BP, *xm = y + (size_t)m * BP;
      for (int v = 0; v < NV; ++v)
      {
        v8d xv;
        SAGE_LOADU(xv, xm + 8 * v);
        for (int u = 0; u < 8; ++u)
        {
          v8d a;
          SAGE_LOADU(a, Tm + u * BP + 8 * v);
          acc[u] += a * xv;
        }
      }
    }
    for (int u = 0; u < 8; ++u)
      z[t0 + u] -= SAGE_HSUM8(acc[u]);
  }
}

// ---- the row passes.  Rows only touch the blocks of their own column ranges, so two row ranges that do not reference each
// other can run on two cores.  A half can also run as the two stages of E.pipe: chain_rows (the chain through row i-1 and
// the diagonal) behind lookahead_rows; rows with an A range are not split (no such rows in the halves of a plan).
enum class RowRole { whole, chain, lookahead }; // factor_rows / chain_rows / lookahead_rows (+ separator_prepass)

// SAGE_CHOL_PROFILE: cycles per bucket (plain aggregate, see RowPrefetch)
struct RowLaps
{
  bool on;
  unsigned long long tp[6], tl;
  inline __attribute__((always_inline)) void lap(int k)
  {
    if (!on)
      return;
    const unsigned long long t_ = __builtin_readcyclecounter();
    tp[k] += t_ - tl;
    tl = t_;
  }
  inline __attribute__((always_inline)) void print(int lo, int hi) const
  {
    if (on)
      fprintf(stderr, "[chol profile] rows %d..%d kcycles: wait %.0f gemm+syrk %.0f apply-inverse %.0f factor+inverse %.0f fwd-subst %.0f other %.0f\n",
              lo, hi, tp[0] * 1e-3, tp[1] * 1e-3, tp[2] * 1e-3, tp[3] * 1e-3, tp[4] * 1e-3, tp[5] * 1e-3);
  }
};
static inline __attribute__((always_inline)) RowLaps row_laps()
{
  static const bool prof = sage::env_flag("SAGE_CHOL_PROFILE");
  return RowLaps{prof, {0, 0, 0, 0, 0, 0}, __builtin_readcyclecounter()};
}

static inline BlockEnvelope::RowPipe *pipe_of(const BlockEnvelope &E, int lo) { return E.pipe + (lo >= E.n1 && E.n1 > 0 ? 1 : 0); }
static inline bool pipe_wait(std::atomic<int> &c, int need) // false: the other stage gave up (negative count)
{
  int v;
  while ((v = c.load(std::memory_order_acquire)) < need)
  {
    if (v < 0)
      return false;
    __builtin_ia32_pause();
  }
  return true;
}

// What every factorising pass ends a row with: the diagonal factor and its inverse, the forward substitution
// y_i = L_ii^-1 (g_i - sum_k L_ik y_k), and the row's publication (pipe->late for the other stage, E.progress for the
// arrow-row tasks).  0, or 1 + i for a non-positive pivot.
template <int NV>
static inline __attribute__((always_inline)) int finish_row(Blocks<NV> blk, double *X, double *y, int i, int lo,
                                                            BlockEnvelope::RowPipe *pipe, RowLaps &laps)
{
  constexpr int BP = NV * 8, BB = BP * BP;
  const BlockEnvelope &E = blk.E;
  laps.lap(1);
  if (!factor_diag<NV>(blk(i, i), X + (size_t)i * BB))
  {
    if (pipe)
      pipe->late.store(-1, std::memory_order_release);
    return 1 + i;
  }
  laps.lap(3);
  const BlockEnvelope::Range rg[2] = {E.a_range(i), E.b_range(i)};
  double w[BP];
  for (int r = 0; r < BP; ++r)
    w[r] = y[(size_t)i * BP + r];
  for (int r = 0; r < 2; ++r)
    for (int k = rg[r].lo; k < rg[r].hi; ++k)
      fwd_sub_block<NV>(w, blk(i, k), y + (size_t)k * BP);
  apply_diag_inverse<NV>(y + (size_t)i * BP, w, X + (size_t)i * BB);
  laps.lap(4);
  if (pipe)
    pipe->late.store(i + 1 - lo, std::memory_order_release);
  if (E.progress && i < E.n1 + E.n2)
    E.progress[i >= E.n1 ? 1 : 0].store(i + 1, std::memory_order_release);
  return 0;
}

// factorise rows [lo, hi) ascending and forward-substitute y, one thread
template <int NV>
static inline __attribute__((always_inline)) int factor_rows(const BlockEnvelope &E, double *T, double *X, double *y,
                                                             int lo, int hi)
{
  constexpr int BB = NV * 8 * NV * 8;
  const Blocks<NV> blk{E, T};
  RowLaps laps = row_laps();
  for (int i = lo; i < hi; ++i)
  {
    laps.lap(5);
    // separator row of a plain split window: its blocks against a half's columns may have been formed already by that
    // half's look-ahead thread (sep_pre) -- tickets, fill and arithmetic; they are skipped below
    BlockEnvelope::Range pre[2] = {{0, 0}, {0, 0}};
    if (E.sep_pre && E.pipe && i >= E.n1 + E.n2)
      for (int hf = 0; hf < 2; ++hf)
      {
        int v;
        while ((v = E.pipe[hf].pre.load(std::memory_order_acquire)) == 1)
          __builtin_ia32_pause();
        if (v < 0)
          return -2;
        if (v == 2)
          pre[hf] = E.sep_range(i, hf);
      }
    if (E.ready && !wait_row_tickets(E, i, T, pre[0].hi > pre[0].lo ? pre[0].hi : 0, pre[1].lo, pre[1].hi))
      return -2;
    laps.lap(0);
    const BlockEnvelope::Range rg[2] = {E.a_range(i), E.b_range(i)}; // the column ranges of row i, in ascending order
    RowPrefetch pf{nullptr, nullptr};
    if (i + 1 < hi)
      pf = row_prefetch<NV>(E, T, i + 1);
    for (int r = 0; r < 2; ++r)
      for (int j = rg[r].lo; j < rg[r].hi; ++j)
      {
        if ((j >= pre[0].lo && j < pre[0].hi) || (j >= pre[1].lo && j < pre[1].hi))
          continue; // (formed by the half's look-ahead thread: same operations, same order)
        double *CT = blk(i, j);
        for (int rk = 0; rk <= r; ++rk)
          for (int k = rg[rk].lo; k < std::min(rg[rk].hi, j); ++k)
            if (E.has(j, k))
              tn_sub<NV>(CT, blk(j, k), blk(i, k), false, pf);
        laps.lap(1);
        apply_inverse<NV>(CT, X + (size_t)j * BB);
        laps.lap(2);
      }
    double *S = blk(i, i);
    for (int r = 0; r < 2; ++r)
      for (int k = rg[r].lo; k < rg[r].hi; ++k)
        tn_sub<NV>(S, blk(i, k), blk(i, k), true, pf);
    if (const int rc = finish_row<NV>(blk, X, y, i, lo, nullptr, laps))
      return rc;
  }
  laps.print(lo, hi);
  return 0;
}

// the second stage of a piped half: for row i the chain that needs row i-1 -- block (i, i-1), its share of the diagonal,
// the diagonal factor and the forward substitution
template <int NV>
static inline __attribute__((always_inline)) int chain_rows(const BlockEnvelope &E, double *T, double *X, double *y,
                                                            int lo, int hi)
{
  constexpr int BB = NV * 8 * NV * 8;
  const Blocks<NV> blk{E, T};
  const int32_t *row_first = E.row_first;
  BlockEnvelope::RowPipe *pipe = pipe_of(E, lo);
  RowLaps laps = row_laps();
  RowPrefetch pf{nullptr, nullptr};
  for (int i = lo; i < hi; ++i)
  {
    laps.lap(5);
    laps.lap(0);
    if (!pipe_wait(pipe->early, i + 1 - lo))
      return -2;
    if (i - 1 >= row_first[i])
    {
      double *CT = blk(i, i - 1);
      if (i - 2 >= row_first[i] && E.has(i - 1, i - 2))
        tn_sub<NV>(CT, blk(i - 1, i - 2), blk(i, i - 2), false, pf);
      apply_inverse<NV>(CT, X + (size_t)(i - 1) * BB);
      tn_sub<NV>(blk(i, i), CT, CT, true, pf);
    }
    if (const int rc = finish_row<NV>(blk, X, y, i, lo, pipe, laps))
      return rc;
  }
  laps.print(lo, hi);
  return 0;
}

// Separator pre-pass (r05, the tail of the look-ahead stage of rows [lo, hi)): the blocks L_sj of the separator rows s
// against THIS half's columns j only need rows of this half -- L_sj = (A_sj - sum_{k < j, same range} L_jk L_sk) L_jj^-T --
// and this thread has nothing left to do: it forms them right behind the chain thread's row j instead of the caller forming
// them after both halves have joined.  Per block the same operations in the same order as in the separator pass
// (bit-identical factor).  false: the chain stage gave up, or a ticket did not arrive.
template <int NV>
static inline __attribute__((always_inline)) bool separator_prepass(const BlockEnvelope &E, double *T, double *X, int lo,
                                                                    int hi)
{
  constexpr int BB = NV * 8 * NV * 8;
  const Blocks<NV> blk{E, T};
  const int K = E.K, sep0 = E.n1 + E.n2, half = lo >= E.n1 && E.n1 > 0 ? 1 : 0;
  BlockEnvelope::RowPipe *pipe = pipe_of(E, lo);
  int jlo = hi;
  // the separator rows' blocks were written by the device's DMA and sit in no cache: ask for them now, while the chain
  // thread still works on the rows this pass waits for
  for (int srow = sep0; srow < K; ++srow)
  {
    const BlockEnvelope::Range c = E.sep_range(srow, half);
    if (c.lo < c.hi)
      jlo = std::min(jlo, c.lo);
    for (int j = std::max(c.lo, lo); j < std::min(c.hi, hi); ++j)
    {
      const char *pb = reinterpret_cast<const char *>(blk(srow, j));
      for (size_t o = 0; o < (size_t)BB * sizeof(double); o += 64)
        __builtin_prefetch(pb + o, 1, 3);
    }
  }
  RowPrefetch pf0{nullptr, nullptr};
  for (int j = std::max(jlo, lo); j < hi; ++j)
  {
    if (!pipe_wait(pipe->late, j + 1 - lo)) // row j complete: its blocks and the inverse of its diagonal factor
      return false;
    for (int srow = sep0; srow < K; ++srow)
    {
      const BlockEnvelope::Range c = E.sep_range(srow, half);
      if (j < c.lo || j >= c.hi)
        continue;
      if (!wait_block(E, T, E.index(srow, j)))
        return false;
      double *CT = blk(srow, j);
      for (int k = c.lo; k < j; ++k)
        if (E.has(j, k))
          tn_sub<NV>(CT, blk(j, k), blk(srow, k), false, pf0);
      apply_inverse<NV>(CT, X + (size_t)j * BB);
    }
  }
  return true;
}

// the first stage of a piped half: for row i everything that only needs the rows <= i-2; with E.sep_pre the separator
// pre-pass behind it
template <int NV>
static inline __attribute__((always_inline)) int lookahead_rows(const BlockEnvelope &E, double *T, double *X, double *,
                                                                int lo, int hi)
{
  constexpr int BB = NV * 8 * NV * 8;
  const Blocks<NV> blk{E, T};
  const int32_t *row_first = E.row_first;
  BlockEnvelope::RowPipe *pipe = pipe_of(E, lo);
  RowLaps laps = row_laps();
  auto give_up = [&](bool early_too) {
    if (early_too)
      pipe->early.store(-1, std::memory_order_release);
    if (E.sep_pre)
      pipe->pre.store(-1, std::memory_order_release);
    return -2;
  };
  if (E.sep_pre)
    pipe->pre.store(1, std::memory_order_release); // (before this stage's first `early`: the chain thread cannot finish its half unseen)
  for (int i = lo; i < hi; ++i)
  {
    laps.lap(5);
    if (E.ready && !wait_row_tickets(E, i, T))
      return give_up(true);
    laps.lap(0);
    RowPrefetch pf{nullptr, nullptr};
    if (i + 1 < hi)
      pf = row_prefetch<NV>(E, T, i + 1);
    // needs the rows <= i-2 complete (and its own earlier rows)
    if (!pipe_wait(pipe->late, i - 1 - lo))
      return give_up(false);
    for (int j = row_first[i]; j < i; ++j)
    {
      double *CT = blk(i, j);
      const int kend = j == i - 1 ? i - 2 : j; // (i, i-1): the product with row i-1's last block is the other stage's
      for (int k = row_first[i]; k < kend; ++k)
        if (E.has(j, k))
          tn_sub<NV>(CT, blk(j, k), blk(i, k), false, pf);
      if (j < i - 1)
        apply_inverse<NV>(CT, X + (size_t)j * BB);
    }
    double *S = blk(i, i);
    for (int k = row_first[i]; k < i - 1; ++k)
      tn_sub<NV>(S, blk(i, k), blk(i, k), true, pf);
    while (pf.p < pf.end) // (short rows: the prefetch of the next row's blocks is part of this stage's job)
      pf.step();
    pipe->early.store(i + 1 - lo, std::memory_order_release);
  }
  if (E.sep_pre)
  {
    const bool ok = separator_prepass<NV>(E, T, X, lo, hi);
    pipe->pre.store(ok ? 2 : -1, std::memory_order_release);
    if (!ok)
      return -2;
  }
  laps.print(lo, hi);
  return 0;
}

// back-substitute rows [lo, hi) descending: x_i = L_ii^-T (y_i - sum_{m>i, (m,i) stored} L_mi^T x_m)
template <int NV>
static inline __attribute__((always_inline)) int back_substitute(const BlockEnvelope &E, double *T, double *X, double *y,
                                                                 int lo, int hi)
{
  constexpr int BP = NV * 8, BB = BP * BP;
  const Blocks<NV> blk{E, T};
  for (int i = hi - 1; i >= lo; --i)
  {
    double z[BP];
    for (int t = 0; t < BP; ++t)
      z[t] = y[(size_t)i * BP + t];
    if (E.col_ptr)
      backsub_columns<NV>(z, blk, y, i, E.col_rows + E.col_ptr[i], E.col_ptr[i + 1] - E.col_ptr[i], E.bs_skip_from);
    else
      backsub_columns<NV>(z, blk, y, i, nullptr, E.K - i - 1, E.bs_skip_from);
    const double *Xi = X + (size_t)i * BB;
    v8d zv[NV];
    for (int v = 0; v < NV; ++v)
      SAGE_LOADU(zv[v], z + 8 * v);
    for (int c = 0; c < BP; ++c)
    {
      v8d acc = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int v = c / 8; v < NV; ++v) // X[c][t] = 0 for t < c (stored zeros inside the first vector)
      {
        v8d a;
        SAGE_LOADU(a, Xi + c * BP + 8 * v);
        acc += a * zv[v];
      }
      y[(size_t)i * BP + c] = SAGE_HSUM8(acc);
    }
  }
  return 0;
}

// Separator rows of a partial factorisation (domain decomposition, shard_solve.cpp): the rows [nI, K) get L_ij for
// their columns j < nI; their blocks (i, j), nI <= j <= i, end as the Schur complement C_ij = A_ij - sum_{k<nI} L_ik L_jk^T
// (not factorised) and y_i as c_i = b_i - sum_{k<nI} L_ik y_k.  No A ranges in this storage.
template <int NV>
static inline __attribute__((always_inline)) void block_schur_rows(const BlockEnvelope &E, double *T, double *X, double *y,
                                                                   int nI)
{
  constexpr int BP = NV * 8, BB = BP * BP;
  const Blocks<NV> blk{E, T};
  RowPrefetch pf{nullptr, nullptr};
  for (int i = nI; i < E.K; ++i)
  {
    const int f = E.row_first[i];
    for (int j = f; j < i; ++j)
    {
      double *CT = blk(i, j);
      for (int k = f; k < std::min(j, nI); ++k)
        if (E.has(j, k))
          tn_sub<NV>(CT, blk(j, k), blk(i, k), false, pf);
      if (j < nI)
        apply_inverse<NV>(CT, X + (size_t)j * BB);
    }
    double *S = blk(i, i);
    for (int k = f; k < std::min(i, nI); ++k)
      tn_sub<NV>(S, blk(i, k), blk(i, k), true, pf);
    for (int k = f; k < std::min(i, nI); ++k)
      fwd_sub_block<NV>(y + (size_t)i * BP, blk(i, k), y + (size_t)k * BP);
  }
}

// ---- entry points.  Every template above is inlined into the multi-versioned functions this macro generates (a v8d must
// not cross a call, see SAGE_LOADU): NAME_40 / NAME_24 / NAME_8 for the three padded block sizes (block_kernels_for) and
// NAME_bp, which picks by Bp.
#define SAGE_ARGS(...) __VA_ARGS__
#define SAGE_BLOCK_ENTRY(RET, NAME, PARAMS, ARGS)                                                                          \
  __attribute__((target_clones("avx512f", "avx2", "default"))) static RET NAME##_40 PARAMS { return NAME<5> ARGS; }        \
  __attribute__((target_clones("avx512f", "avx2", "default"))) static RET NAME##_24 PARAMS { return NAME<3> ARGS; }        \
  __attribute__((target_clones("avx512f", "avx2", "default"))) static RET NAME##_8 PARAMS { return NAME<1> ARGS; }         \
  static inline RET NAME##_bp(int Bp, SAGE_ARGS PARAMS)                                                                    \
  {                                                                                                                        \
    return Bp == 40 ? NAME##_40 ARGS : Bp == 24 ? NAME##_24 ARGS : NAME##_8 ARGS;                                          \
  }
static inline bool block_kernels_for(int Bp) { return Bp == 40 || Bp == 24 || Bp == 8; }

#define SAGE_ROWS_PARAMS (const BlockEnvelope &E, double *T, double *X, double *y, int lo, int hi)
SAGE_BLOCK_ENTRY(int, factor_rows, SAGE_ROWS_PARAMS, (E, T, X, y, lo, hi))
SAGE_BLOCK_ENTRY(int, chain_rows, SAGE_ROWS_PARAMS, (E, T, X, y, lo, hi))
SAGE_BLOCK_ENTRY(int, lookahead_rows, SAGE_ROWS_PARAMS, (E, T, X, y, lo, hi))
SAGE_BLOCK_ENTRY(int, back_substitute, SAGE_ROWS_PARAMS, (E, T, X, y, lo, hi))
SAGE_BLOCK_ENTRY(void, block_schur_rows, (const BlockEnvelope &E, double *T, double *X, double *y, int nI), (E, T, X, y, nI))

// ---------------------------------------------------------------------------------------------------------------
// Separator rows on several cores (loop-closure plans, plan_blocks: cover keyframes).  A separator row i has a range in
// the first half (A = [a_first, a_first + a_cnt)), a range in the second half ([row_first, sep0)) and the separator
// columns [sep0, i).  Everything a row does inside ONE half only needs that half's factor and the row's own blocks:
//   task A (row i, half h):  L_ij for the columns j of that range (ascending, following the half's progress counter),
//                            the partial sums  -sum_j L_ij L_ij^T  (diagonal block) and  -sum_j L_ij y_j  (rhs)
//   task B (rows i > i2, half h):  -sum_k L_i2,k L_ik^T over the common columns of the two rows in that half
// all into private buffers; the separator block itself (a handful of rows) is then finished by the caller, who adds the
// partial sums in a fixed order (deterministic: the result does not depend on which thread ran which task).
// ---------------------------------------------------------------------------------------------------------------
struct SepTaskA
{
  int row, half, j0, j1; // columns [j0, j1)
  // r05: a long chain may carry a PARTNER row of the same half and column range (the partner's own entry is a `slave`: its
  // slots are filled by the master's thread): the two rows share the loads of the half's blocks column by column, and the
  // number of long chains fits the cores of the halves' L3 domain (a chain on another domain runs ~30 % slower and the
  // separator then waits a millisecond for it: config 5, 3 cover rows x 2 halves on 4 free cores)
  int partner = -1;
  bool slave = false;
};
// Which long arrow-row chains a thread takes: domain 0 = the caller's L3 domain (first half), 1 = the second half's own L3
// domain of a two-domain placement, -1 = a pool worker elsewhere on the node (short tasks and pair products only)
static thread_local int tl_domain = 0;
struct SepTaskB
{
  int i, i2, half, k0, k1; // common columns [k0, k1), i2 < i
};
struct SepJob
{
  const BlockEnvelope *E = nullptr;
  double *T = nullptr, *X = nullptr, *y = nullptr;
  int sep0 = 0;
  std::vector<SepTaskA> ta;
  std::vector<SepTaskB> tb;
  std::vector<double> wd, Pp; // [ta][Bp], [tb][BB]
  std::atomic<int> nextA{0}, doneA{0}, nextB{0}, doneB{0};
  std::atomic<int> nextLong[2];
  std::vector<int> long_tasks[2], short_tasks; // indices into ta: chains of > 16 columns by half (masters only) / the rest
  std::atomic<int> abort{0};
  std::atomic<int> progress[2];
  // phase C (back substitution): y_i -= sum over the separator rows m of L_mi^T x_m for the rows i of the halves, in
  // chunks of rows -- after the separator rows' x are known (goC: 0 wait, 1 go, 2 skip)
  std::vector<std::pair<int, int>> tc;
  std::atomic<int> goC{0}, nextC{0}, doneC{0};
  double t_start = 0.0; // (SAGE_DEBUG_TIMING)
  int dbg_waits[64] = {};
};

static void sep_job_build(SepJob &J)
{
  const BlockEnvelope &E = *J.E;
  const int sep0 = E.n1 + E.n2, K = E.K, BB = E.Bp * E.Bp;
  J.sep0 = sep0;
  for (int i = sep0; i < K; ++i)
    for (int h = 0; h < 2; ++h)
    {
      const BlockEnvelope::Range c = E.sep_range(i, h);
      if (c.hi > c.lo)
        J.ta.push_back({i, h, c.lo, c.hi});
    }
  // longest first: the long arrow rows start early, the short middle-separator rows fill the gaps
  std::stable_sort(J.ta.begin(), J.ta.end(), [](const SepTaskA &x, const SepTaskA &y) { return x.j1 - x.j0 > y.j1 - y.j0; });
  {
    // pair long chains of the same half and range until they fit the fast threads (the pool workers on the caller's L3
    // domain + the caller and the second half's helper join only after their halves: not counted)
    const bool two = g_two_domains.load(std::memory_order_acquire);
    const int fast0 = g_domain_threads[0].load(std::memory_order_acquire), fast1 = g_domain_threads[1].load(std::memory_order_acquire);
    auto is_long = [&](const SepTaskA &a) { return a.j1 - a.j0 > 16; };
    int n_long[2] = {0, 0};
    for (auto &a : J.ta)
      if (is_long(a))
        ++n_long[a.half];
    // capacity per half: its own domain's workers (two domains), or the one domain's workers shared by both halves
    auto over = [&](int h) {
      if (fast0 <= 0)
        return false;
      return two ? n_long[h] > std::max(1, h == 0 ? fast0 : fast1) : n_long[0] + n_long[1] > fast0;
    };
    if (!sage::env_flag("SAGE_SOLVE_NO_PAIRING"))
      for (size_t t = 0; t < J.ta.size(); ++t)
      {
        SepTaskA &a = J.ta[t];
        if (!is_long(a) || a.slave || a.partner >= 0 || !over(a.half))
          continue;
        for (size_t u = J.ta.size(); u-- > t + 1;) // (the last rows first: they are the ones that used to end up off-domain)
        {
          SepTaskA &b = J.ta[u];
          if (is_long(b) && !b.slave && b.partner < 0 && b.half == a.half && b.j0 >= a.j0 && b.j1 == a.j1)
          {
            a.partner = (int)u;
            b.slave = true;
            --n_long[a.half];
            break;
          }
        }
      }
    J.nextLong[0].store(0, std::memory_order_relaxed);
    J.nextLong[1].store(0, std::memory_order_relaxed);
    for (size_t t = 0; t < J.ta.size(); ++t)
      if (!J.ta[t].slave)
      {
        if (is_long(J.ta[t]))
          J.long_tasks[J.ta[t].half].push_back((int)t);
        else
          J.short_tasks.push_back((int)t);
      }
  }
  // (i2 == i, r05: the row's own  sum_k L_ik L_ik^T  -- its share of the diagonal block -- as pair products too: it is not on
  //  the chain's recurrence, and one product less per column lets the arrow-row chains keep closer to the halves)
  for (int i = sep0; i < K; ++i)
    for (int i2 = sep0; i2 <= i; ++i2)
      for (int h = 0; h < 2; ++h)
      {
        const BlockEnvelope::Range c = E.sep_range(i, h), c2 = E.sep_range(i2, h);
        const int k0 = std::max(c.lo, c2.lo), k1 = std::min(c.hi, c2.hi);
        // (pieces of <= 64 columns: the pair products of two long arrow rows spread over the whole pool)
        for (int c0 = k0; c0 < k1; c0 += 64)
          J.tb.push_back({i, i2, h, c0, std::min(k1, c0 + 64)});
      }
  std::stable_sort(J.tb.begin(), J.tb.end(), [](const SepTaskB &x, const SepTaskB &y) { return x.k1 - x.k0 > y.k1 - y.k0; });
  J.wd.assign(J.ta.size() * (size_t)E.Bp, 0.0);
  J.Pp.assign(J.tb.size() * (size_t)BB, 0.0);
  J.progress[0].store(0, std::memory_order_relaxed);
  J.progress[1].store(E.n1, std::memory_order_relaxed);
  if (E.col_ptr)
    for (int r0 = 0; r0 < sep0; r0 += 32)
      J.tc.push_back({r0, std::min(sep0, r0 + 32)});
}

template <int NV>
static inline __attribute__((always_inline)) void sep_run_c(SepJob &J, int t)
{
  constexpr int BP = NV * 8;
  const BlockEnvelope &E = *J.E;
  const Blocks<NV> blk{E, J.T};
  for (int i = J.tc[t].first; i < J.tc[t].second; ++i)
  {
    const int n0 = E.col_ptr[i], n1 = E.col_ptr[i + 1];
    int q0 = n0;
    while (q0 < n1 && E.col_rows[q0] < J.sep0)
      ++q0;
    if (q0 == n1)
      continue;
    backsub_columns<NV>(J.y + (size_t)i * BP, blk, J.y, i, E.col_rows + q0, n1 - q0, 0x7fffffff);
  }
}

template <int NV>
static inline __attribute__((always_inline)) void sep_run_a(SepJob &J, int t)
{
  constexpr int BP = NV * 8, BB = BP * BP;
  const BlockEnvelope &E = *J.E;
  double *T = J.T, *X = J.X, *y = J.y;
  const Blocks<NV> blk{E, T};
  const SepTaskA &a = J.ta[t];
  // the rows this thread carries: the task's own and, for a paired chain, its partner's (same half, same columns)
  const int rows[2] = {a.row, a.partner >= 0 ? J.ta[a.partner].row : -1};
  const int row_j0[2] = {a.j0, a.partner >= 0 ? J.ta[a.partner].j0 : 0}; // (a partner may join at a later column)
  double *wds[2] = {J.wd.data() + (size_t)t * BP, a.partner >= 0 ? J.wd.data() + (size_t)a.partner * BP : nullptr};
  RowPrefetch pf{nullptr, nullptr};
  for (int j = a.j0; j < a.j1; ++j)
  {
    // the half's row j (its blocks, X_j and y_j) must be final
    unsigned spins = 0;
    while (J.progress[a.half].load(std::memory_order_acquire) <= j)
    {
      __builtin_ia32_pause();
      if ((++spins & 0xff) == 0 && J.abort.load(std::memory_order_acquire))
        return;
    }
    if (spins)
      ++J.dbg_waits[t & 63]; // (SAGE_DEBUG_TIMING: columns at which this chain had caught up with its half)
    if (j + 1 < a.j1)
    {
      // the half's row j + 1 (a half row: no A range) and its inverse: asked for now, used next column
      const RowPrefetch next = row_prefetch<NV>(E, T, j + 1);
      pf.p2 = next.p;
      pf.end2 = next.end;
      pf.p3 = reinterpret_cast<const char *>(X + (size_t)(j + 1) * BB);
      pf.end3 = pf.p3 + BB * sizeof(double);
    }
    for (int q = 0; q < 2 && rows[q] >= 0; ++q)
    {
      const int i = rows[q];
      if (j < row_j0[q])
        continue;
      if (!wait_block(E, T, E.index(i, j), &J.abort)) // this block of row i has arrived from the device (or is fill)
        return;
      double *CT = blk(i, j);
      if (j + 1 < a.j1)
      {
        pf.p = reinterpret_cast<const char *>(blk(i, j + 1));
        pf.end = pf.p + BB * sizeof(double);
      }
      for (int k = std::max(row_j0[q], (int)E.row_first[j]); k < j; ++k) // (row j is a half row: its columns are [row_first[j], j])
        if (E.has(j, k))
          tn_sub<NV>(CT, blk(j, k), blk(i, k), false, pf);
      apply_inverse<NV>(CT, X + (size_t)j * BB);
      // (the diagonal share  sum_j CT_j CT_j^T  is a pair product of phase B since r05: not on this chain's recurrence)
      fwd_sub_block<NV>(wds[q], CT, y + (size_t)j * BP);
    }
  }
}

template <int NV>
static inline __attribute__((always_inline)) void sep_run_b(SepJob &J, int t)
{
  constexpr int BB = NV * 8 * NV * 8;
  const Blocks<NV> blk{*J.E, J.T};
  const SepTaskB &b = J.tb[t];
  double *P = J.Pp.data() + (size_t)t * BB;
  RowPrefetch pf{nullptr, nullptr};
  for (int k = b.k0; k < b.k1; ++k)
    tn_sub<NV>(P, blk(b.i2, k), blk(b.i, k), b.i2 == b.i, pf); // (a row with itself: the upper triangle is all the factorisation reads)
}

// the separator block: rows [sep0, K) with the partial sums of the tasks folded in; then their back substitution
template <int NV>
static inline __attribute__((always_inline)) int sep_finish(SepJob &J)
{
  constexpr int BP = NV * 8, BB = BP * BP;
  const BlockEnvelope &E = *J.E;
  double *T = J.T, *X = J.X, *y = J.y;
  const Blocks<NV> blk{E, T};
  const int sep0 = J.sep0, K = E.K;
  auto add_pair_products = [&](double *C, int i, int i2) { // fixed order: deterministic
    for (size_t t = 0; t < J.tb.size(); ++t)
      if (J.tb[t].i == i && J.tb[t].i2 == i2)
      {
        const double *P = J.Pp.data() + t * BB;
        for (int o = 0; o < BB; ++o)
          C[o] += P[o];
      }
  };
  RowPrefetch pf{nullptr, nullptr};
  for (int i = sep0; i < K; ++i)
  {
    // (the blocks of the columns < sep0 went through the arrow-row tasks one by one)
    if (E.ready && !wait_row_tickets(E, i, T, sep0))
      return -2;
    const int c0 = std::max((int)E.row_first[i], sep0);
    for (int j = c0; j < i; ++j)
    {
      double *CT = blk(i, j);
      add_pair_products(CT, i, j);
      for (int k = std::max(c0, std::max((int)E.row_first[j], sep0)); k < j; ++k)
        tn_sub<NV>(CT, blk(j, k), blk(i, k), false, pf);
      apply_inverse<NV>(CT, X + (size_t)j * BB);
    }
    double *S = blk(i, i);
    double w[BP];
    for (int r = 0; r < BP; ++r)
      w[r] = y[(size_t)i * BP + r];
    add_pair_products(S, i, i); // the row's own pair products
    for (size_t t = 0; t < J.ta.size(); ++t)
      if (J.ta[t].row == i)
      {
        const double *wd = J.wd.data() + t * BP;
        for (int r = 0; r < BP; ++r)
          w[r] += wd[r];
      }
    for (int k = c0; k < i; ++k)
    {
      tn_sub<NV>(S, blk(i, k), blk(i, k), true, pf);
      fwd_sub_block<NV>(w, blk(i, k), y + (size_t)k * BP);
    }
    if (!factor_diag<NV>(S, X + (size_t)i * BB))
      return 1 + i;
    apply_diag_inverse<NV>(y + (size_t)i * BP, w, X + (size_t)i * BB);
  }
  return 0;
}

SAGE_BLOCK_ENTRY(void, sep_run_a, (SepJob &J, int t), (J, t))
SAGE_BLOCK_ENTRY(void, sep_run_b, (SepJob &J, int t), (J, t))
SAGE_BLOCK_ENTRY(void, sep_run_c, (SepJob &J, int t), (J, t))
SAGE_BLOCK_ENTRY(int, sep_finish, (SepJob &J), (J))

static bool debug_timing() // SAGE_DEBUG_TIMING
{
  static const bool on = sage::env_flag("SAGE_DEBUG_TIMING");
  return on;
}

// run fn(q) for every ticket q < n this thread draws from `next`
template <class F>
static inline void take_tasks(std::atomic<int> &next, int n, F fn)
{
  for (int q; (q = next.fetch_add(1, std::memory_order_acq_rel)) < n;)
    fn(q);
}

// take tasks until none is left (called by the pool's workers, the helper after its half, and the caller).  Long chains go
// to the threads of the halves' L3 domains only (tl_domain >= 0), longest first; everybody takes the short ones.
static void sep_work(SepJob &J)
{
  const int nA = (int)J.ta.size(), nB = (int)J.tb.size();
  const bool dbg_a = debug_timing();
  auto run_a = [&](int t) {
    const double ta0 = dbg_a ? mono_seconds() : 0.0;
    if (!J.abort.load(std::memory_order_acquire))
      sep_run_a_bp(J.E->Bp, J, t);
    if (dbg_a && J.ta[t].j1 - J.ta[t].j0 > 16)
      fprintf(stderr, "[sage arrow task] row %d%s half %d cols %d: %.0f us on cpu %d (ends %.0f us after job start; caught up with its half at %d columns)\n",
              J.ta[t].row, J.ta[t].partner >= 0 ? " (+ a partner row)" : "", J.ta[t].half, J.ta[t].j1 - J.ta[t].j0,
              1e6 * (mono_seconds() - ta0), sched_getcpu(), 1e6 * (mono_seconds() - J.t_start), J.dbg_waits[t & 63]);
    J.doneA.fetch_add(J.ta[t].partner >= 0 ? 2 : 1, std::memory_order_acq_rel);
  };
  if (tl_domain >= 0)
  {
    // its own half's chains first; then whatever is left of the other half's (a chain nobody has started is better run
    // across domains than not at all: liveness does not depend on the placement)
    const int first = g_two_domains.load(std::memory_order_acquire) ? (tl_domain & 1) : 0;
    for (int pass = 0; pass < 2; ++pass)
    {
      const int h = pass == 0 ? first : 1 - first;
      take_tasks(J.nextLong[h], (int)J.long_tasks[h].size(), [&](int q) { run_a(J.long_tasks[h][q]); });
    }
  }
  take_tasks(J.nextA, (int)J.short_tasks.size(), [&](int q) { run_a(J.short_tasks[q]); });
  while (J.doneA.load(std::memory_order_acquire) < nA) // phase B reads the rows phase A completes
    __builtin_ia32_pause();
  take_tasks(J.nextB, nB, [&](int t) {
    if (!J.abort.load(std::memory_order_acquire))
      sep_run_b_bp(J.E->Bp, J, t);
    J.doneB.fetch_add(1, std::memory_order_acq_rel);
  });
}

// phase C: entered by the pool's workers right after sep_work (they wait for the caller's go), by the caller when the
// separator rows are back-substituted
static void sep_work_c(SepJob &J, bool wait_for_go)
{
  if (wait_for_go)
  {
    int g;
    while ((g = J.goC.load(std::memory_order_acquire)) == 0)
      __builtin_ia32_pause();
    if (g != 1)
      return;
  }
  take_tasks(J.nextC, (int)J.tc.size(), [&](int t) {
    sep_run_c_bp(J.E->Bp, J, t);
    J.doneC.fetch_add(1, std::memory_order_acq_rel);
  });
}

static inline void cpu_relax() { __builtin_ia32_pause(); }

// Worker pool for the arrow rows (host_threads.h Worker, n threads): woken by block_chol_arm(true), spins for a job for
// 20 ms at most.  A caller that owns the pool (`busy`) hands its SepJob over through posted / open / active.
struct SepPool final : Worker
{
  explicit SepPool(int n) : Worker(n, 20e-3) {}
  std::atomic<bool> open{false};
  std::atomic<int> active{0};
  std::atomic<bool> busy{false};
  std::atomic<SepJob *> job{nullptr};
  void run(int t) override
  {
    // hand-off: the owner does `open = false` THEN reads `active`; a worker does `active += 1` THEN reads `open`.
    // A store followed by a load of another variable needs sequential consistency on both sides (with release /
    // acquire the two may be reordered -- the owner reads active == 0 while a late worker still reads open == true
    // and runs a job that lives on the owner's stack after the owner has returned)
    active.fetch_add(1, std::memory_order_seq_cst);
    if (open.load(std::memory_order_seq_cst))
    {
      SepJob *j = job.load(std::memory_order_acquire);
      tl_domain = th[t].dom.load(std::memory_order_acquire);
      sep_work(*j);
      sep_work_c(*j, true);
    }
    active.fetch_sub(1, std::memory_order_seq_cst);
  }
  bool hold() const override { return open.load(std::memory_order_acquire); } // (an open job keeps the pool armed)
};
static std::atomic<SepPool *> g_sep_pool_made{nullptr}; // (the placement monitor must not CREATE the pool by asking for it)
static SepPool *sep_pool()
{
  static SepPool *p = [] {
    const unsigned hw = std::thread::hardware_concurrency();
    // (r04: the halves run two threads each now, so the arrow-row tasks are what the halves wait for -- config 5 per LM
    //  step with 4 / 6 / 10 / 14 workers: 7.3 / 6.9 / 6.55 / 6.5 ms on one box)
    int n = getenv("SAGE_SOLVE_POOL") ? atoi(getenv("SAGE_SOLVE_POOL")) : 10;
    n = std::min(n, (int)hw - 4);
    if (n < 1)
      return (SepPool *)nullptr;
    SepPool *q = new SepPool(n);
    g_sep_pool_made.store(q, std::memory_order_release);
    return q;
  }();
  return p;
}

// factorise and forward-substitute rows [lo, hi) / back-substitute them, with the kernels of the envelope's block size
static int block_chol_range(const BlockEnvelope &E, double *T, double *X, double *y, int lo, int hi,
                            RowRole role = RowRole::whole)
{
  return role == RowRole::whole   ? factor_rows_bp(E.Bp, E, T, X, y, lo, hi)
         : role == RowRole::chain ? chain_rows_bp(E.Bp, E, T, X, y, lo, hi)
                                  : lookahead_rows_bp(E.Bp, E, T, X, y, lo, hi);
}
static int block_back_range(const BlockEnvelope &E, double *T, double *X, double *y, int lo, int hi)
{
  return back_substitute_bp(E.Bp, E, T, X, y, lo, hi);
}

// Helper threads of a split window: [0] takes the second half, [1] / [2] are the look-ahead stages of the first / second
// half (BlockEnvelope::RowPipe).  A helper (host_threads.h Worker, one thread) is woken by block_chol_arm() (called while
// the caller still waits for the device), then spins for a job for 8 ms at most so that picking one up costs no wake-up
// latency.  Nobody depends on a helper that has not claimed its job: the second half is claimed back and run by the
// caller, a half without a look-ahead stage runs as one thread.
struct CholHelper final : Worker
{
  explicit CholHelper(int kind_) : Worker(1, 8e-3), kind(kind_) {}
  std::atomic<int> claim{0};   // 0 free, 1 helper, 2 caller
  std::atomic<int> p1_rc{-2};  // result of the helper's factorisation pass (-2: not finished)
  std::atomic<int> go_p2{0};   // 1: run the back substitution, 2: skip it
  std::atomic<int> p2_done{0};
  std::atomic<bool> busy{false}; // one client at a time
  const BlockEnvelope *E = nullptr;
  double *T = nullptr, *X = nullptr, *y = nullptr;
  const int kind; // 0: second half (factorisation, later the back substitution), 1: look-ahead stage of rows [lo, hi)
  int lo = 0, hi = 0;
  void run(int) override;
};
static CholHelper *chol_helper(int idx = 0)
{
  // the objects live for the life of the process (host_threads.h); their threads come and go
  static CholHelper **hs = [] {
    CholHelper **v = new CholHelper *[3]{nullptr, nullptr, nullptr};
    const unsigned hc = std::thread::hardware_concurrency();
    for (int i = 0; i < 3; ++i)
      if (hc >= (i == 0 ? 2u : 4u))
        v[i] = new CholHelper(i == 0 ? 0 : 1);
    return v;
  }();
  return hs[idx];
}

static std::atomic<long long> g_lookahead_count{0};

// rows [lo, hi) can run as two stages: plain band rows (no A range, nothing left of lo)
static bool rows_can_pipe(const BlockEnvelope &E, int lo, int hi)
{
  static const bool off = sage::env_flag("SAGE_SOLVE_NO_LOOKAHEAD");
  if (off || E.no_lookahead || !E.pipe || hi - lo < 4)
    return false;
  for (int i = lo; i < hi; ++i)
    if ((E.a_cnt && E.a_cnt[i]) || E.row_first[i] < lo)
      return false;
  return true;
}

// hand rows [lo, hi) to look-ahead helper `idx`; true once the helper has claimed the job (it then WILL publish its
// progress in E.pipe), false when there is no armed helper or it did not answer within a few microseconds
static bool lookahead_engage(int idx, const BlockEnvelope &E, double *T, double *X, double *y, int lo, int hi)
{
  CholHelper *h = chol_helper(idx);
  if (!h || !h->armed.load(std::memory_order_acquire) || !rows_can_pipe(E, lo, hi))
    return false;
  bool expect = false;
  if (!h->busy.compare_exchange_strong(expect, true, std::memory_order_acq_rel))
    return false;
  h->E = &E; h->T = T; h->X = X; h->y = y; h->lo = lo; h->hi = hi;
  h->p1_rc.store(-2, std::memory_order_relaxed);
  h->claim.store(0, std::memory_order_release); // (a helper still looking at an older post claims only after the fields are set)
  h->posted.fetch_add(1, std::memory_order_release);
  const double t0 = mono_seconds();
  unsigned spins = 0;
  while (h->claim.load(std::memory_order_acquire) == 0)
  {
    cpu_relax();
    if ((++spins & 63) == 0 && mono_seconds() - t0 > 20e-6)
    {
      int e0 = 0;
      if (h->claim.compare_exchange_strong(e0, 2, std::memory_order_acq_rel))
      {
        h->busy.store(false, std::memory_order_release);
        return false;
      }
    }
  }
  g_lookahead_count.fetch_add(1, std::memory_order_relaxed);
  return true;
}
// ---- the second half on helper 0.  helper_engage: post the job to the armed helper (null: none armed, or another caller
// owns it).  Nobody depends on a helper that has not claimed its job: after its own half the caller asks helper_claimed --
// true: the helper runs the half and WILL publish its result (helper_join_factor), false: the job is claimed back and the
// caller runs the half itself.  helper_go_back / helper_join_back: the same for the half's back substitution (only for a
// claimed job); helper_release sends the helper back to sleep until the next arm and frees it for other callers.
static CholHelper *helper_engage(const BlockEnvelope &E, double *T, double *X, double *y)
{
  CholHelper *h = chol_helper();
  if (!h || !h->armed.load(std::memory_order_acquire))
    return nullptr;
  bool expect = false;
  if (!h->busy.compare_exchange_strong(expect, true, std::memory_order_acq_rel))
    return nullptr;
  h->E = &E; h->T = T; h->X = X; h->y = y;
  h->p1_rc.store(-2, std::memory_order_relaxed);
  h->go_p2.store(0, std::memory_order_relaxed);
  h->p2_done.store(0, std::memory_order_relaxed);
  h->claim.store(0, std::memory_order_release);
  h->posted.fetch_add(1, std::memory_order_release);
  return h;
}
static bool helper_claimed(CholHelper *h)
{
  int expect = 0;
  return !h->claim.compare_exchange_strong(expect, 2, std::memory_order_acq_rel);
}
static int helper_join_factor(CholHelper *h)
{
  int rc;
  while ((rc = h->p1_rc.load(std::memory_order_acquire)) == -2)
    cpu_relax();
  return rc;
}
static void helper_go_back(CholHelper *h, bool run) { h->go_p2.store(run ? 1 : 2, std::memory_order_release); }
static void helper_join_back(CholHelper *h)
{
  while (!h->p2_done.load(std::memory_order_acquire))
    cpu_relax();
}
static void helper_release(CholHelper *h)
{
  h->armed.store(false, std::memory_order_release);
  h->busy.store(false, std::memory_order_release);
}
// the look-ahead stage of lookahead_engage(idx) == true: wait for its result, then as helper_release
static void lookahead_release(int idx)
{
  helper_join_factor(chol_helper(idx));
  helper_release(chol_helper(idx));
}

// ---- the arrow-row pool.  pool_engage: hand the job to the armed pool (null: no pool, not armed, or another caller owns
// it -- the caller then runs every task itself).  pool_release: close the job and wait until no worker is inside it (the
// job lives on the caller's stack; see SepPool::run for why this pair is sequentially consistent).
static SepPool *pool_engage(SepJob &job)
{
  SepPool *pool = sep_pool();
  if (!pool || !pool->armed.load(std::memory_order_acquire))
    return nullptr;
  bool expect = false;
  if (!pool->busy.compare_exchange_strong(expect, true, std::memory_order_acq_rel))
    return nullptr;
  pool->job.store(&job, std::memory_order_release);
  pool->open.store(true, std::memory_order_seq_cst);
  pool->posted.fetch_add(1, std::memory_order_release);
  return pool;
}
static void pool_release(SepPool *pool)
{
  pool->open.store(false, std::memory_order_seq_cst);
  while (pool->active.load(std::memory_order_seq_cst) != 0)
    cpu_relax();
  pool->armed.store(false, std::memory_order_release);
  pool->busy.store(false, std::memory_order_release);
}

// the separator rows of a loop-closure plan, after both halves (rc: their result): the caller takes tasks too (all of them
// when no pool thread is around), then finishes the separator block
static int arrow_separator(SepJob &job, int rc, double t_halves)
{
  if (rc != 0)
    job.abort.store(1, std::memory_order_release);
  sep_work(job);
  while (job.doneB.load(std::memory_order_acquire) < (int)job.tb.size())
    cpu_relax();
  if (debug_timing())
    fprintf(stderr, "[sage block chol] arrow tasks (%zu row chains, %zu pair products) done %.0f us after the halves\n",
            job.ta.size(), job.tb.size(), 1e6 * (mono_seconds() - t_halves));
  if (rc == 0 && job.abort.load(std::memory_order_acquire))
    rc = -2;
  return rc ? rc : sep_finish_bp(job.E->Bp, job);
}

// the separator rows' share of every half row's back substitution, in row chunks on the pool (the arrow rows put three
// more blocks into every column: streaming them once, in parallel, instead of inside the two sequential sweeps); the
// halves' own sweeps then leave the separator rows out (E.bs_skip_from)
static void arrow_back_substitute(SepJob &job, BlockEnvelope &E, int rc)
{
  const bool par_c = rc == 0 && !job.tc.empty();
  job.goC.store(par_c ? 1 : 2, std::memory_order_release);
  if (!par_c)
    return;
  sep_work_c(job, false);
  while (job.doneC.load(std::memory_order_acquire) < (int)job.tc.size())
    cpu_relax();
  E.bs_skip_from = job.sep0;
}

void CholHelper::run(int)
{
  int expect = 0;
  if (!claim.compare_exchange_strong(expect, 1, std::memory_order_acq_rel))
    return;
  const BlockEnvelope &e = *E;
  if (kind == 1)
  {
    const int rc = block_chol_range(e, T, X, y, lo, hi, RowRole::lookahead);
    p1_rc.store(rc == -2 ? -3 : rc, std::memory_order_release); // (-2 is the "not finished" value)
    return;
  }
  const bool piped = lookahead_engage(2, e, T, X, y, e.n1, e.n1 + e.n2);
  const int rc = block_chol_range(e, T, X, y, e.n1, e.n1 + e.n2, piped ? RowRole::chain : RowRole::whole);
  if (piped)
    lookahead_release(2);
  p1_rc.store(rc, std::memory_order_release);
  int g;
  while ((g = go_p2.load(std::memory_order_acquire)) == 0)
    cpu_relax();
  if (g == 1)
    block_back_range(e, T, X, y, e.n1, e.n1 + e.n2);
  p2_done.store(1, std::memory_order_release);
}
} // namespace

Worker *solve_worker(int idx, bool make)
{
  if (idx < 3)
    return chol_helper(idx);
  return make ? sep_pool() : g_sep_pool_made.load(std::memory_order_acquire);
}

// ---- the plan: its two predicates and the elimination-order planner need nothing but the standard library (no thread,
// no atomic, no vector unit); they live here because the storage they lay out is the storage the solver above reads.

// rows of the separator part whose ranges run far along a half (> 16 columns): the chains the pool's fast threads carry
int block_plan_long_arrow_chains(const BlockEnvelope &E)
{
  int n = 0;
  if (E.n1 > 0 && E.n2 > 0 && E.a_cnt)
    for (int i = E.n1 + E.n2; i < E.K; ++i)
      for (int h = 0; h < 2; ++h)
        n += E.sep_range(i, h).hi - E.sep_range(i, h).lo > 16 ? 1 : 0;
  return n;
}

bool block_plan_has_arrow_rows(const BlockEnvelope &E)
{
  long long reach = 0;
  if (E.n1 > 0 && E.n2 > 0 && E.a_cnt)
    for (int i = E.n1 + E.n2; i < E.K; ++i)
      for (int h = 0; h < 2; ++h)
        reach += E.sep_range(i, h).hi - E.sep_range(i, h).lo;
  return reach > 64; // (a plain split window: <= 2 x 3 blocks per separator row)
}

int plan_blocks(int K, const std::vector<std::pair<int, int>> &links, bool may_split, BlockPlan &out)
{
  std::vector<int32_t> &perm = out.perm, &pos = out.pos, &row_first = out.row_first, &row_off = out.row_off,
                       &a_first = out.a_first, &a_cnt = out.a_cnt, &a_off = out.a_off, &blk_row = out.blk_row,
                       &blk_col = out.blk_col, &blk_src = out.blk_src;
  int &n1 = out.n1, &n2 = out.n2, &nblk = out.nblk;
  // ---- elimination order.  A chain-like window (every keyframe linked to a few predecessors) splits at a separator of
  // w consecutive keyframes into two halves without a link between them: order = [first half ascending | second half
  // DESCENDING | separator].  The two halves are then two independent banded factorisations (the host runs them on two
  // cores), only the w separator rows see both.  Windows with long-range links (loop closures) keep the identity order.
  perm.assign(K, 0);
  pos.assign(K, 0);
  for (int k = 0; k < K; ++k)
    perm[k] = k;
  n1 = n2 = 0;
  for (auto &l : links)
    if (l.first < 0 || l.second <= l.first || l.second >= K)
      return SAGE_E_INVALID;
  if (may_split && K >= 16)
  {
    // the helper's half runs a little slower than the caller's (it wakes from sleep for every solve): give it
    // `bias` rows less
    constexpr int bias = 1;
    // Loop closures: a link that spans more than a separator's width crosses every candidate split.  Such links are
    // covered by a small set C of keyframes (greedy: the keyframe on most still-uncovered long links first) that joins
    // the separator: order = [first half | second half descending | middle separator | C].  The rows of C are "arrow"
    // rows -- their ranges run the whole length of both halves -- but the two halves stay two independent banded
    // factorisations, and the arrow rows are independent of each other until the (small) separator block: the host
    // factorisation spreads them over a few cores (block_chol_solve_tr).  At most 8 cover keyframes; otherwise, and
    // for windows without a split point, the identity order stays.
    std::vector<char> inC(K, 0);
    std::vector<int> cover;
    int best_m = -1, best_w = 0;
    for (;;)
    {
      int best_cost = 2 * K;
      best_m = -1;
      for (int m = K / 4; m <= (3 * K) / 4; ++m)
      {
        int wdt = 0;
        for (auto &l : links)
          if (!inC[l.first] && !inC[l.second] && l.first < m && l.second >= m)
            wdt = std::max(wdt, l.second - m + 1);
        if (wdt < 1 || wdt > 8 || m + wdt > K - 2)
          continue;
        const int cost = std::max(m, K - m - wdt + bias) + 2 * wdt;
        if (cost < best_cost)
        {
          best_cost = cost;
          best_m = m;
          best_w = wdt;
        }
      }
      if (best_m > 0 || cover.size() >= 8)
        break;
      // no split point: cover one more long link (span > 8: it cannot sit inside a separator)
      std::vector<int> deg(K, 0);
      int any = 0;
      for (auto &l : links)
        if (!inC[l.first] && !inC[l.second] && l.second - l.first > 8)
        {
          ++deg[l.first];
          ++deg[l.second];
          ++any;
        }
      if (!any)
        break;
      const int pick = (int)(std::max_element(deg.begin(), deg.end()) - deg.begin()); // (first maximum: lowest keyframe)
      inC[pick] = 1;
      cover.push_back(pick);
    }
    if (best_m > 0)
    {
      int q = 0;
      for (int k = 0; k < best_m; ++k)
        if (!inC[k])
          perm[q++] = k;
      n1 = q;
      for (int k = K - 1; k >= best_m + best_w; --k)
        if (!inC[k])
          perm[q++] = k;
      n2 = q - n1;
      for (int k = best_m; k < best_m + best_w; ++k)
        if (!inC[k])
          perm[q++] = k;
      std::sort(cover.begin(), cover.end());
      for (int k : cover)
        perm[q++] = k;
      if (n1 < 1 || n2 < 1) // (degenerate: everything on one side) -> identity order
      {
        for (int k = 0; k < K; ++k)
          perm[k] = k;
        n1 = n2 = 0;
      }
    }
  }
  for (int q = 0; q < K; ++q)
    pos[perm[q]] = q;
  // block storage: row i keeps the envelope range B = [row_first[i], i]; a separator row additionally keeps a range
  // A = [a_first[i], n1) over the tail of the first half (the columns in between -- the whole second half up to its
  // own tail -- are structurally zero in the factor and are neither stored nor visited).
  const bool split = n1 > 0;
  const int sep0 = n1 + n2;
  row_first.assign(K, 0);
  row_off.assign(K, 0);
  a_first.assign(K, 0);
  a_cnt.assign(K, 0);
  a_off.assign(K, 0);
  for (int k = 0; k < K; ++k)
  {
    row_first[k] = k;
    a_first[k] = n1;
  }
  for (auto &l : links)
  {
    const int i = std::max(pos[l.first], pos[l.second]), j = std::min(pos[l.first], pos[l.second]);
    if (split && i >= sep0 && j < n1)
      a_first[i] = std::min(a_first[i], j);
    else
      row_first[i] = std::min(row_first[i], j);
  }
  if (split)
    for (int i = sep0; i < K; ++i)
    {
      row_first[i] = std::min(row_first[i], (int32_t)sep0); // separator rows couple through both halves
      a_cnt[i] = n1 - a_first[i];
    }
  nblk = 0;
  for (int k = 0; k < K; ++k)
  {
    a_off[k] = nblk;
    nblk += a_cnt[k];
    row_off[k] = nblk;
    nblk += k - row_first[k] + 1;
  }
  blk_row.assign(nblk, 0);
  blk_col.assign(nblk, 0);
  blk_src.assign(nblk, -1);
  for (int k = 0; k < K; ++k)
  {
    for (int j = a_first[k]; j < a_first[k] + a_cnt[k]; ++j)
    {
      blk_row[out.index(k, j)] = k;
      blk_col[out.index(k, j)] = j;
    }
    for (int j = row_first[k]; j <= k; ++j)
    {
      blk_row[out.index(k, j)] = k;
      blk_col[out.index(k, j)] = j;
    }
  }
  // column lists (rows below the diagonal that store a block of the column, ascending)
  out.col_ptr.assign(K + 1, 0);
  for (int b = 0; b < nblk; ++b)
    if (blk_row[b] != blk_col[b])
      ++out.col_ptr[blk_col[b] + 1];
  for (int j = 0; j < K; ++j)
    out.col_ptr[j + 1] += out.col_ptr[j];
  out.col_rows.assign(std::max(1, (int)out.col_ptr[K]), 0);
  {
    std::vector<int32_t> fill(out.col_ptr.begin(), out.col_ptr.end() - 1);
    for (int k = 0; k < K; ++k) // rows ascending -> every column's list comes out ascending
    {
      for (int j = a_first[k]; j < a_first[k] + a_cnt[k]; ++j)
        out.col_rows[fill[j]++] = k;
      for (int j = row_first[k]; j < k; ++j)
        out.col_rows[fill[j]++] = k;
    }
  }
  for (size_t l = 0; l < links.size(); ++l)
  {
    const int a = links[l].first, b = links[l].second;
    const int i = std::max(pos[a], pos[b]), j = std::min(pos[a], pos[b]);
    int &src = blk_src[out.index(i, j)];
    if (src >= 0)
      return SAGE_E_UNSUPPORTED; // duplicate link: the host path accumulates, this one does not
    // the packed link block is H[a rows][b cols]; block (i,j) is H[perm[i] rows][perm[j] cols]
    src = (int)l | (perm[i] == a ? 0x40000000 : 0);
  }
  return SAGE_OK;
}

int block_chol_partial(const BlockEnvelope &E, double *T, double *X, double *y, int nI)
{
  if (!block_kernels_for(E.Bp) || E.a_cnt)
    return -1;
  const int rc = block_chol_range(E, T, X, y, 0, nI); // interior rows: factor + forward substitution
  if (rc)
    return rc;
  block_schur_rows_bp(E.Bp, E, T, X, y, nI);
  return 0;
}

int block_chol_partial_back(const BlockEnvelope &E, double *T, double *X, double *y, int nI)
{
  if (!block_kernels_for(E.Bp) || E.a_cnt)
    return -1;
  return block_back_range(E, T, X, y, 0, nI); // x_i for the interior rows, y[nI..K) holding the separators' x
}

int block_chol_solve_tr(const BlockEnvelope &E0, double *T, double *X, double *y)
{
  if (!block_kernels_for(E0.Bp))
    return -1;
  const int K = E0.K;
  if (E0.n1 <= 0 || E0.n2 <= 0)
  {
    const int rc = block_chol_range(E0, T, X, y, 0, K);
    return rc ? rc : block_back_range(E0, T, X, y, 0, K);
  }
  const int sep0 = E0.n1 + E0.n2;
  // ---- engage.  Loop-closure plans: the long separator rows are cut into tasks for the worker pool (SepJob); the halves
  // publish their progress so that the tasks run right behind them
  BlockEnvelope E = E0;
  const bool arrow = block_plan_has_arrow_rows(E0);
  SepJob job;
  SepPool *pool = nullptr;
  if (arrow)
  {
    job.E = &E; job.T = T; job.X = X; job.y = y;
    sep_job_build(job);
    job.t_start = mono_seconds();
    E.progress = job.progress;
    pool = pool_engage(job);
  }
  BlockEnvelope::RowPipe pipes[2];
  E.pipe = pipes;
  static const bool no_sep_pre = sage::env_flag("SAGE_SOLVE_NO_SEP_PRE");
  E.sep_pre = !arrow && !no_sep_pre;
  CholHelper *h = helper_engage(E, T, X, y);
  // ---- the first half, as two stages when its look-ahead helper answers (the second half's thread asks for its own)
  const bool piped = lookahead_engage(1, E, T, X, y, 0, E.n1);
  const bool dbg = debug_timing();
  double tp[6] = {0, 0, 0, 0, 0, 0};
  auto lap = [&](int k) { // (SAGE_DEBUG_TIMING)
    if (dbg)
      tp[k] = mono_seconds();
  };
  lap(0);
  int rc = block_chol_range(E, T, X, y, 0, E.n1, piped ? RowRole::chain : RowRole::whole);
  if (piped)
    lookahead_release(1);
  lap(1);
  // ---- join the second half: the helper's result, or run it here
  const bool helper_has_it = h && helper_claimed(h);
  const int rc2 = helper_has_it ? helper_join_factor(h) : rc == 0 ? block_chol_range(E, T, X, y, E.n1, sep0) : 0;
  lap(2);
  if (rc == 0)
    rc = rc2;
  // ---- the separator rows (arrow or plain) and their back substitution
  if (arrow)
    rc = arrow_separator(job, rc, tp[2]);
  else if (rc == 0)
    rc = block_chol_range(E, T, X, y, sep0, K);
  if (rc == 0)
    block_back_range(E, T, X, y, sep0, K);
  if (arrow)
  {
    arrow_back_substitute(job, E, rc);
    if (pool)
      pool_release(pool);
  }
  lap(3);
  // ---- back substitution of the halves
  if (helper_has_it)
    helper_go_back(h, rc == 0);
  if (rc == 0)
  {
    block_back_range(E, T, X, y, 0, E.n1);
    if (!helper_has_it)
      block_back_range(E, T, X, y, E.n1, sep0);
  }
  lap(4);
  if (helper_has_it)
    helper_join_back(h);
  lap(5);
  if (dbg)
    fprintf(stderr, "[sage block chol] us: first half %.0f (+wait for the %s %.0f) separator %.0f%s back-subst %.0f (+wait %.0f)\n",
            1e6 * (tp[1] - tp[0]), helper_has_it ? "helper" : "second half, same thread", 1e6 * (tp[2] - tp[1]),
            1e6 * (tp[3] - tp[2]), arrow ? (pool ? " (arrow rows, worker pool)" : " (arrow rows, no pool)") : "",
            1e6 * (tp[4] - tp[3]), 1e6 * (tp[5] - tp[4]));
  // ---- release
  if (h)
    helper_release(h);
  return rc;
}

BlockEnvelope envelope_of(const BlockPlan &plan, int Bp)
{
  BlockEnvelope env;
  env.K = (int)plan.row_first.size(); env.Bp = Bp; env.n1 = plan.n1; env.n2 = plan.n2;
  env.row_first = plan.row_first.data(); env.row_off = plan.row_off.data();
  env.a_first = plan.a_first.data(); env.a_cnt = plan.a_cnt.data(); env.a_off = plan.a_off.data();
  env.col_ptr = plan.col_ptr.data(); env.col_rows = plan.col_rows.data();
  return env;
}
} // namespace sage

extern "C" long long sage_solve_lookahead_count(void) { return sage::g_lookahead_count.load(); }

namespace sage
{
int block_system_build(const double *packed, int K, int nlinks, const int32_t *links, int B, double damp, const double *diag_add,
                       const double *g_add, BlockPlan &bp, std::vector<double> &T, std::vector<double> &y)
{
  const int Bp = padded_block(B);
  if (Bp == 0)
    return SAGE_E_UNSUPPORTED;
  const int BB = B * B, BBp = Bp * Bp;
  const double *diag = packed;
  const double *lnk = diag + (size_t)K * BB;
  const double *g = lnk + (size_t)nlinks * BB;
  std::vector<std::pair<int, int>> lk(nlinks);
  for (int l = 0; l < nlinks; ++l)
    lk[l] = {links[2 * l], links[2 * l + 1]}; // (plan_blocks refuses a link that is not a < b inside the window)
  // transposed-block storage (the one the window engine runs on the device-scattered storage), with the same
  // elimination order and two-core split
  int rcp = plan_blocks(K, lk, !env_flag("SAGE_SOLVE_NO_SPLIT"), bp);
  if (rcp == SAGE_E_UNSUPPORTED) // duplicate links accumulate on this path: plan without them
  {
    std::sort(lk.begin(), lk.end());
    lk.erase(std::unique(lk.begin(), lk.end()), lk.end());
    rcp = plan_blocks(K, lk, !env_flag("SAGE_SOLVE_NO_SPLIT"), bp);
  }
  if (rcp != SAGE_OK)
    return rcp;
  // per keyframe, then per link: a link listed twice accumulates (damped_system.h has the element rules)
  T.assign((size_t)bp.nblk * BBp, 0.0);
  y.assign((size_t)K * Bp, 0.0);
  for (int q = 0; q < K; ++q)
  {
    const int k = bp.perm[q];
    double *D = T.data() + (size_t)bp.index(q, q) * BBp;
    for (int r = 0; r < Bp; ++r)
      for (int c = 0; c < Bp; ++c)
        D[stored_slot(r, c, Bp)] =
            (r < B && c < B) ? damped_diag_elem(diag + (size_t)k * BB, B, r, c, diag_add ? diag_add[k * B + r] : 0.0, damp)
                             : damped_pad_elem(r, c, damp);
    for (int r = 0; r < B; ++r)
      y[(size_t)q * Bp + r] = damped_rhs_elem(g[(size_t)k * B + r], g_add ? g_add[k * B + r] : 0.0);
  }
  for (int l = 0; l < nlinks; ++l)
  {
    const int a = links[2 * l], b = links[2 * l + 1];
    const int qi = std::max(bp.pos[a], bp.pos[b]), qj = std::min(bp.pos[a], bp.pos[b]);
    double *D = T.data() + (size_t)bp.index(qi, qj) * BBp;
    const bool row_is_a = bp.perm[qi] == a;
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c)
        D[stored_slot(r, c, Bp)] += lnk[(size_t)l * BB + link_elem(row_is_a, r, c, B)];
  }
  return SAGE_OK;
}

int block_system_factor(const BlockPlan &bp, int Bp, double *T, double *X, double *y)
{
  BlockEnvelope env = envelope_of(bp, Bp);
  SolveLease lease; // (arm and solve: no shutdown joins a helper in between)
  if (bp.n1 > 0)
    env.no_lookahead = block_chol_arm(block_plan_has_arrow_rows(env), block_plan_long_arrow_chains(env));
  return block_chol_solve_tr(env, T, X, y);
}
} // namespace sage

extern "C" int sage_block_solve(const double *packed, int K, int nlinks, const int32_t *links, int B, double damp,
                                const double *diag_add, const double *g_add, double *delta)
{
  if (!packed || K < 1 || B < 1 || nlinks < 0 || (nlinks > 0 && !links) || !delta)
    return SAGE_E_INVALID;
  // the factorisation works on blocks padded to Bp rows (identity on the padding): the fixed-block kernels' sizes
  const int Bp = sage::padded_block(B);
  sage::BlockPlan bp;
  std::vector<double> T, y;
  if (const int rcb = sage::block_system_build(packed, K, nlinks, links, B, damp, diag_add, g_add, bp, T, y))
    return rcb;
  std::vector<double> X((size_t)K * Bp * Bp);
  static const bool dbg = sage::env_flag("SAGE_DEBUG_TIMING");
  const auto t0 = std::chrono::steady_clock::now();
  const int rcf = sage::block_system_factor(bp, Bp, T.data(), X.data(), y.data());
  if (dbg)
    fprintf(stderr, "[sage block_solve] fixed-block Cholesky + substitution %.3f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  if (rcf != 0)
    return SAGE_E_NOT_PSD;
  for (int k = 0; k < K; ++k)
    std::memcpy(delta + (size_t)k * B, y.data() + (size_t)bp.pos[k] * Bp, sizeof(double) * B);
  return SAGE_OK;
}
