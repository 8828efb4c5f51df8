// solve_kernels.hip -- damped Gauss-Newton/LM step of the keyframe window: the hybrid solve (gfx950 + host cores).
//
// Replaces, for the batched window engine, the host side of the reference's optimisation step: the normal
// equations the factors hand to the solver (core/gtsam/photometric_factor.cpp:106-219 -> gtsam HessianFactor,
// ISAM2 update, core/mapping/mapper.cpp:118-156) and the LM damping policy of camera_tracker.cpp:1182
// (H + damp*diag(H)), followed by the manifold retraction of gtsam_traits.h:45-70.  The window's block normal
// equations are keyframe blocks of B = 7+CS rows, coupled along factor-graph links:
//
//   scatter   packed [K diag blocks | link blocks | gradient] (double, HBM)  ->  block-envelope storage of the lower
//             triangle (+ priors, LM damping, identity padding to Bp rows: damped_system.h), streamed into pinned host
//             memory in the order the factorisation consumes it, a ticket per block.  The blocks hold the SOLVER rows
//             only: Bs <= B of them when every keyframe holds a whole group (window_plan.h: solver_rows)
//   factor    fixed-block Cholesky + substitutions on host cores (block_solver.cpp: block_chol_solve_tr -- two halves and
//             a separator, each half as two pipelined stages)
//   retract   candidate variables = retract(current, delta), read zero-copy from the host's solution
//
// Everything is double: cond(H_damped) ~ 1e9 on the headline window.
//
// Why the factorisation is on the host: it is a dependency chain of K*B = 2.5 k pivots with ~27 M fused multiply-adds
// in total.  A device factorisation in one workgroup took 4.2 ms on MI355X (K = 64, B = 39; removed in r04), AVX-512 host
// cores do the same work in 0.13 ms.  The block storage (3.2 MB) crosses PCIe overlapped with the factorisation.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "block_solver.h"
#include "device_buffers.h"
#include "damped_system.h"
#include "host_math.h"
#include "sage_device.h"
#include "sage_internal.h"
#include "window_plan.h"

namespace sage
{

struct SolvePlan
{
  int K, B, Bs, Bp, nblk, nlinks; // B rows per keyframe in the packed buffer, Bs of them in the solver, padded to Bp
  const int32_t *row_first; // [K] first block column of block row i
  const int32_t *row_off;   // [K] index of block (i, row_first[i]) in the block storage
  const int32_t *blk_row, *blk_col, *blk_src; // [nblk]; src = link index (bit 30: the row keyframe is the link's first
                                               // end) or -1
  const int32_t *perm, *pos; // elimination order: perm[position] = keyframe, pos[keyframe] = position
  const int32_t *hold;       // [K] masks of held variables (sage_window_hold), or null: nothing is held
  const int32_t *to_block, *to_solver; // [Bs] solver row -> block row, [B] block row -> solver row or -1 (dropped)
};

// Head of the pinned result block; the candidate variables [K*VS floats] and the delta [K*B doubles] follow it.
struct SolveResult
{
  double step_norm2; // |delta|^2
  int status;        // 0 candidate written, 1 no candidate (the host aborted the solve: non-positive pivot / error), 2 the
                     // host's word never came -- the caller then treats the evaluation as failed instead of reading a
                     // stale candidate
  unsigned go;       // the host's word to the pre-launched retract (solve_retract_kernel)
};
static size_t result_vars_offset() { return sizeof(SolveResult); }
static size_t result_delta_offset(int K, int VS) { return (sizeof(SolveResult) + (size_t)K * VS * sizeof(float) + 15) / 16 * 16; }

// Workgroups of the scatter kernel.  Not measured against other counts on record; r04 measured the kernel itself at this
// count (88 -> 73 us with one system-scope release per block).
constexpr int kScatterWorkgroups = 32;

// ------------------------------------------------------------------------------------------------
// scatter: a few workgroups walk the blocks in the order the host factorisation consumes them and write straight into
// pinned host memory: every block is followed by a ticket in `flags`, so the host starts on row 0 while the later rows
// are still crossing PCIe.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void solve_scatter_kernel(const SolvePlan P, const double *__restrict__ packed,
                                                            const float *__restrict__ vars0, int VS, int CS,
                                                            const SolvePriors pri, double damp,
                                                            double *__restrict__ L, double *__restrict__ y,
                                                            const int32_t *__restrict__ order, unsigned *flags,
                                                            unsigned epoch)
{
  const int tid = threadIdx.x;
  const int B = P.B, Bs = P.Bs, Bp = P.Bp, BB = B * B;
  __shared__ double s_dadd[64], s_gadd[64]; // per solver row (Bs <= Bp <= 40)
  __shared__ int s_row[64];                 // the block row behind it (damped_system.h: solver rows)
  if (tid < Bs)
    s_row[tid] = P.to_block[tid];
  __syncthreads();
  for (int it = blockIdx.x; it < P.nblk; it += gridDim.x)
  {
    const int b = order[it];
    const int i = P.blk_row[b], j = P.blk_col[b], srcf = P.blk_src[b];
    const int src = srcf < 0 ? -1 : (srcf & 0x3fffffff);
    const bool row_is_a = srcf >= 0 && (srcf & 0x40000000);
    if (src < 0 && i != j)
      continue; // structural fill-in: the host zeroes it at its first touch (BlockEnvelope::fill) -- nothing to deliver
    const int kf = P.perm[i]; // keyframe of this block row
    const int hold_r = P.hold ? P.hold[kf] : 0, hold_c = P.hold ? P.hold[P.perm[j]] : 0; // (damped_system.h: held variables)
    const double *diag = packed + (size_t)kf * BB;
    const double *lnk = packed + (size_t)P.K * BB + (size_t)(src < 0 ? 0 : src) * BB;
    const double *g = packed + (size_t)P.K * BB + (size_t)P.nlinks * BB + (size_t)kf * B;
    double *out = L + (size_t)b * Bp * Bp;
    if (i == j)
    {
      const float *var = vars0 + (size_t)kf * VS; // pose 12, scale, code CS
      if (tid < Bs)
      {
        double da, ga;
        prior_row(pri, kf, s_row[tid], CS, var, var[12], var + 13, da, ga, hold_r);
        s_dadd[tid] = da;
        s_gadd[tid] = ga;
      }
      __syncthreads();
    }
    // consecutive threads write consecutive doubles (the stores are crossing PCIe)
    for (int o = tid; o < Bp * Bp; o += blockDim.x)
    {
      const int c = o / Bp, r = o - c * Bp; // o == stored_slot(r, c, Bp)
      double v = 0.0;
      const bool in = r < Bs && c < Bs;
      const bool held = in && solver_elem_held(hold_r, hold_c, s_row, r, c, CS);
      if (i == j)
        v = in ? (held ? held_diag_elem(r, c) : solver_diag_elem(diag, B, s_row, r, c, s_dadd[r], damp))
               : damped_pad_elem(r, c, damp);
      else if (in && !held)
        v = lnk[solver_link_elem(row_is_a, s_row, r, c, B)];
      out[o] = v;
    }
    if (i == j)
      for (int r = tid; r < Bp; r += blockDim.x)
        y[(size_t)i * Bp + r] =
            (r < Bs && !(hold_r && row_held(hold_r, s_row[r], CS))) ? damped_rhs_elem(g[s_row[r]], s_gadd[r]) : 0.0;
    // the block (and its rhs rows) are visible to the host before the ticket is: the workgroup barrier orders every
    // lane's stores before lane 0's system-scope release (one cache write-back per block instead of one per wave)
    __syncthreads();
    if (tid == 0)
    {
      __threadfence_system();
      *reinterpret_cast<volatile unsigned *>(flags + b) = epoch;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// retract: candidate = current (+) delta   (damped_system.h pose_retract; tangent order [trans, rot], left update)
// ------------------------------------------------------------------------------------------------
// One workgroup.  Besides the candidate variables (device) it writes the host mirror -- candidate variables, delta and
// |delta|^2 -- straight into pinned host memory (h_*: device-visible), so no copy follows the solve.
// (1024 threads: x lives in pinned host memory -- every read is a PCIe round trip, so the kernel's time is the number of
// sequential reads per thread)
__global__ __launch_bounds__(1024) void solve_retract_kernel(const double *__restrict__ x, int K, int B, int Bp, int CS,
                                                            int VS, const int32_t *__restrict__ pos,
                                                            const int32_t *__restrict__ hold,
                                                            const int32_t *__restrict__ to_solver,
                                                            const float *__restrict__ vars0,
                                                            float *__restrict__ vars1, float *__restrict__ h_vars,
                                                            double *__restrict__ h_delta, SolveResult *h_res,
                                                            unsigned epoch)
{
  const int tid = threadIdx.x;
  const volatile unsigned *go = &h_res->go;
  // The kernel is enqueued BEFORE the host factorises (right behind the scatter) and waits here for the host's word in
  // pinned memory: the solution is there (go == epoch), or there is none (bit 31 set: non-positive pivot / abort).  The
  // launch latency of a kernel issued into an idle queue (tens of microseconds on the step's critical path) is hidden
  // behind the factorisation.  A watchdog (2 s of the 100 MHz wall clock) ends the wait if the host never answers.
  __shared__ int s_go;
  if (tid == 0)
  {
    const unsigned long long t0 = wall_clock64();
    unsigned v;
    bool timed_out = false;
    for (;;)
    {
      v = *go;
      // the word carries the epoch of the LAST solve the host answered: mine -> go / abort (bit 31); a NEWER one (the host
      // gave up on this solve -- its own word was overwritten before this kernel ran) -> abort; an older one -> keep waiting
      const unsigned d = ((v & 0x7fffffffu) - epoch) & 0x7fffffffu;
      if (d == 0u)
        break;
      if (d < 0x40000000u && (v & 0x7fffffffu) != 0u)
      {
        v = 0x80000000u;
        break;
      }
      __builtin_amdgcn_s_sleep(4);
      if (wall_clock64() - t0 > 200000000ull)
      {
        v = 0x80000000u;
        timed_out = true;
        break;
      }
    }
    __threadfence_system();
    s_go = (v & 0x80000000u) ? 0 : 1;
    volatile int *status = &h_res->status;
    *status = timed_out ? 2 : (s_go ? 0 : 1);
  }
  __syncthreads();
  if (!s_go)
    return;
  double nrm = 0.0;
  for (int idx = tid; idx < K * B; idx += blockDim.x)
  {
    const int k = idx / B, r = idx - k * B;
    // delta exactly zero, the entry copied bit for bit (a row the solver dropped is a row every keyframe holds)
    const bool held = hold && row_held(hold[k], r, CS);
    const double d = held ? 0.0 : x[(size_t)pos[k] * Bp + to_solver[r]]; // x: elimination order, solver rows
    h_delta[idx] = d;
    nrm += d * d;
    const float *v0 = vars0 + (size_t)k * VS;
    if (r >= 6)
    {
      const int slot = r < 6 + CS ? 13 + r - 6 : 12; // code entries, then the scale
      const float v = held ? v0[slot] : v0[slot] + (float)d; // (x + -0.0f may flip a sign bit)
      vars1[(size_t)k * VS + slot] = v;
      h_vars[(size_t)k * VS + slot] = v;
    }
  }
  for (int k = tid; k < K; k += blockDim.x)
  {
    const double *xk = x + (size_t)pos[k] * Bp;
    const float *v0 = vars0 + (size_t)k * VS;
    float *o = vars1 + (size_t)k * VS; // the device candidate; the host mirror gets its copy
    if (hold && (hold[k] & kHoldPose)) // (se3_exp of a zero delta is not the identity in fp32)
      for (int i = 0; i < 12; ++i)
        o[i] = v0[i];
    else
    {
      float d6[6];
      for (int i = 0; i < 6; ++i)
        d6[i] = (float)xk[to_solver[i]];
      pose_retract(v0, d6, o);
    }
    for (int i = 0; i < 12; ++i)
      h_vars[(size_t)k * VS + i] = o[i];
  }
  __shared__ double s_n[16];
  for (int off = 32; off > 0; off >>= 1)
    nrm += __shfl_down(nrm, off);
  if ((tid & 63) == 0)
    s_n[tid >> 6] = nrm;
  __syncthreads();
  if (tid == 0)
  {
    double tot = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) // fixed order
      tot += s_n[w];
    h_res->step_norm2 = tot;
  }
}

// ------------------------------------------------------------------------------------------------
// host side: plan + launcher
// ------------------------------------------------------------------------------------------------
struct DeviceSolver
{
  int K = 0, B = 0, Bs = 0, Bp = 0, nblk = 0, nlinks = 0, VS = 0;
  sage_rt::DevBuf d_int;       // all int tables in one allocation
  sage_rt::DevBuf d_hold;      // [K] masks of held variables (solver_set_holds), or empty
  sage_rt::PinnedBuf h_pinned; // [SolveResult | K*VS floats | K*B doubles]
  sage_rt::PinnedBuf h_T;      // one allocation: block storage, then the right-hand side, then the tickets
  double *h_y = nullptr;
  unsigned *h_flags = nullptr; // a ticket (the epoch of the solve that wrote it) per block
  unsigned epoch = 0, go_epoch = 0;
  SolvePlan plan{};
  const int32_t *d_order = nullptr; // the blocks in the order the host factorisation consumes them
  std::vector<double> h_X;          // inverses of the diagonal factors
  BlockPlan host_plan;              // elimination order and block storage (what the host factorisation reads)
  std::vector<uint8_t> h_fill;      // per block: structural fill-in (not delivered by the scatter kernel: BlockEnvelope::fill)
  bool factor_valid = false;        // h_T / h_X hold the factor of solve number `epoch`, damped by factor_damp (solver_factor)
  double factor_damp = 0.0;

  double *h_blocks() const { return h_T.as<double>(); }
  SolveResult *result() const { return h_pinned.as<SolveResult>(); }
  float *host_vars() const { return reinterpret_cast<float *>(h_pinned.as<char>() + result_vars_offset()); }
  double *host_delta() const { return reinterpret_cast<double *>(h_pinned.as<char>() + result_delta_offset(K, VS)); }
};

int solver_create(DeviceSolver **out, int K, const plan::SolverRows &rows, int VS,
                  const std::vector<std::pair<int, int>> &links, hipStream_t stream)
{
  *out = nullptr;
  const int B = rows.B, Bs = rows.Bs;
  const int Bp = sage::padded_block(Bs);
  if (Bp == 0 || K < 1)
    return SAGE_E_UNSUPPORTED;
  BlockPlan bp;
  const int rcp = plan_blocks(K, links, !sage::env_flag("SAGE_SOLVE_NO_SPLIT"), bp);
  if (rcp != SAGE_OK)
    return rcp;
  const int n1 = bp.n1, n2 = bp.n2, nblk = bp.nblk;
  const std::vector<int32_t> &perm = bp.perm, &pos = bp.pos, &row_first = bp.row_first, &row_off = bp.row_off,
                             &a_cnt = bp.a_cnt, &a_off = bp.a_off, &blk_row = bp.blk_row, &blk_col = bp.blk_col,
                             &blk_src = bp.blk_src;
  std::unique_ptr<DeviceSolver> S(new DeviceSolver); // (an early return releases what has been allocated so far)
  S->K = K; S->B = B; S->Bs = Bs; S->Bp = Bp; S->nblk = nblk; S->nlinks = (int)links.size(); S->VS = VS;
  // one allocation for the int tables
  std::vector<int32_t> all;
  auto put = [&](const std::vector<int32_t> &v) {
    const size_t off = all.size();
    all.insert(all.end(), v.begin(), v.end());
    while (all.size() % 4)
      all.push_back(0);
    return off;
  };
  const size_t o_rf = put(row_first), o_ro = put(row_off), o_br = put(blk_row), o_bc = put(blk_col),
               o_bs = put(blk_src), o_pm = put(perm), o_ps = put(pos);
  // consumption order of the host factorisation: the two halves row by row side by side, the separator last
  std::vector<int32_t> order;
  auto push_row = [&](int i) {
    for (int q = 0; q < a_cnt[i]; ++q)
      order.push_back(a_off[i] + q);
    for (int q = 0; q <= i - row_first[i]; ++q)
      order.push_back(row_off[i] + q);
  };
  if (n1 > 0)
  {
    for (int t = 0; t < std::max(n1, n2); ++t)
    {
      if (t < n1)
        push_row(t);
      if (t < n2)
        push_row(n1 + t);
    }
    for (int i = n1 + n2; i < K; ++i)
      push_row(i);
  }
  else
    for (int i = 0; i < K; ++i)
      push_row(i);
  const size_t o_ord = put(order);
  const size_t o_tb = put(rows.to_block), o_ts = put(rows.to_solver);
  if (S->d_int.reserve(all.size() * sizeof(int32_t)))
    return (int)hipErrorOutOfMemory;
  if (hipMemcpyAsync(S->d_int.p, all.data(), all.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess)
    return (int)hipErrorUnknown;
  if (hipStreamSynchronize(stream) != hipSuccess)
    return (int)hipErrorUnknown;
  const size_t ty_doubles = (size_t)nblk * Bp * Bp + (size_t)K * Bp;
  if (S->h_T.reserve(ty_doubles * sizeof(double) + (size_t)nblk * sizeof(unsigned)))
    return (int)hipErrorOutOfMemory;
  S->h_y = S->h_blocks() + (size_t)nblk * Bp * Bp;
  S->h_flags = reinterpret_cast<unsigned *>(S->h_blocks() + ty_doubles);
  std::memset(S->h_flags, 0, (size_t)nblk * sizeof(unsigned));
  S->h_X.assign((size_t)K * Bp * Bp, 0.0);
  const size_t h_bytes = result_delta_offset(K, VS) + (size_t)K * B * sizeof(double);
  if (S->h_pinned.reserve(h_bytes))
    return (int)hipErrorOutOfMemory;
  std::memset(S->h_pinned.p, 0, h_bytes);
  const int32_t *base = S->d_int.as<int32_t>();
  SolvePlan &P = S->plan;
  P.K = K; P.B = B; P.Bs = Bs; P.Bp = Bp; P.nblk = nblk; P.nlinks = (int)links.size();
  P.row_first = base + o_rf; P.row_off = base + o_ro;
  P.blk_row = base + o_br; P.blk_col = base + o_bc; P.blk_src = base + o_bs; P.perm = base + o_pm; P.pos = base + o_ps;
  P.to_block = base + o_tb; P.to_solver = base + o_ts;
  S->d_order = base + o_ord;
  S->h_fill.assign((size_t)nblk, 0);
  for (int b = 0; b < nblk; ++b)
    S->h_fill[b] = (blk_src[b] < 0 && blk_row[b] != blk_col[b]) ? 1 : 0;
  S->host_plan = std::move(bp); // (last: the tables above are references into it)
  *out = S.release();
  return SAGE_OK;
}

void solver_destroy(DeviceSolver *S) { delete S; }

// the window's held variables: [K] masks (damped_system.h); the scatter and the retract apply them from the next solve on
int solver_set_holds(DeviceSolver *S, const std::vector<uint8_t> &hold, hipStream_t stream)
{
  if ((int)hold.size() != S->K)
    return SAGE_E_INVALID;
  const std::vector<int32_t> masks(hold.begin(), hold.end());
  if (S->d_hold.reserve(masks.size() * sizeof(int32_t)))
    return (int)hipErrorOutOfMemory;
  if (hipMemcpyAsync(S->d_hold.p, masks.data(), masks.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return (int)hipErrorUnknown;
  S->plan.hold = S->d_hold.as<int32_t>();
  return SAGE_OK;
}

// enqueue scatter and retract, factorise on the host in between (the retract waits on the device for the host's word);
// the candidate's host mirror is valid once the stream has drained (or a later kernel's ticket has been seen).
// The dependency chain of the factorisation runs on host cores, everything around it stays on the device: the scatter
// kernel streams the blocks into pinned host memory in the order the factorisation consumes them and tickets each one,
// so the host works on row 0 while the rest is still crossing PCIe (no D2H copy, no stream sync).
int solver_run(DeviceSolver *S, hipStream_t stream, const double *packed_dev, const float *vars0, float *vars1,
               int CS, double damp, const SolvePriors &pri)
{
  static const bool dbgt = sage::env_flag("SAGE_DEBUG_TIMING");
  hipError_t eh;
  // held from the arm until block_chol_solve_tr returns, also without a split (the solve may still hand work to helpers
  // another caller armed): no shutdown joins a helper in between
  SolveLease lease;
  BlockEnvelope env = envelope_of(S->host_plan, S->Bp);
  // the helper core (and, for loop-closure plans with long separator rows, the worker pool) wakes up while this
  // thread waits for the device
  if (env.n1 > 0)
    env.no_lookahead = block_chol_arm(block_plan_has_arrow_rows(env), block_plan_long_arrow_chains(env));
  S->epoch += 1;
  if (S->epoch == 0) // wrapped: 0 is the "never written" value
    S->epoch = 1;
  S->factor_valid = false; // (the scatter below overwrites the last solve's factor)
  hipLaunchKernelGGL(solve_scatter_kernel, dim3(std::min(kScatterWorkgroups, S->nblk)), dim3(256), 0, stream, S->plan,
                     packed_dev, vars0, S->VS, CS, pri, damp, S->h_blocks(), S->h_y, S->d_order,
                     S->h_flags, S->epoch);
  if ((eh = hipGetLastError()) != hipSuccess)
    return (int)eh;
  // the retract right behind the scatter: it waits on the device for this thread's word (solve_retract_kernel)
  volatile unsigned *go = &S->result()->go;
  S->go_epoch = (S->go_epoch + 1) & 0x7fffffffu;
  if (S->go_epoch == 0)
    S->go_epoch = 1;
  hipLaunchKernelGGL(solve_retract_kernel, dim3(1), dim3(1024), 0, stream, S->h_y, S->K, S->B, S->Bp, CS, S->VS,
                     S->plan.pos, S->plan.hold, S->plan.to_solver, vars0, vars1, S->host_vars(), S->host_delta(),
                     S->result(), S->go_epoch);
  if ((eh = hipGetLastError()) != hipSuccess)
    return (int)eh;
  struct GoGuard // whatever happens below, the waiting kernel gets its word
  {
    volatile unsigned *go;
    unsigned word;
    ~GoGuard()
    {
      std::atomic_thread_fence(std::memory_order_release);
      *go = word;
    }
  } guard{go, S->go_epoch | 0x80000000u};
  const auto t1 = std::chrono::steady_clock::now();
  env.ready = S->h_flags; env.epoch = S->epoch;
  env.fill = S->h_fill.data();
  const int bad = block_chol_solve_tr(env, S->h_blocks(), S->h_X.data(), S->h_y);
  const auto t2 = std::chrono::steady_clock::now();
  if (dbgt)
    fprintf(stderr, "[sage hybrid solve] wait for the system + host cholesky %.3f ms\n",
            std::chrono::duration<double, std::milli>(t2 - t1).count());
  if (bad == -2)
    return SAGE_E_STATE; // the device never delivered a block (see block_chol_solve_tr)
  if (bad)
    return SAGE_E_NOT_PSD;
  guard.word = S->go_epoch; // the solution is in h_y: go
  S->factor_valid = true;
  S->factor_damp = damp;
  return SAGE_OK;
}

const float *solver_host_vars(const DeviceSolver *S) { return S->host_vars(); }
const double *solver_host_delta(const DeviceSolver *S) { return S->host_delta(); }
double solver_host_step_norm2(const DeviceSolver *S) { return S->result()->step_norm2; }
int solver_host_status(const DeviceSolver *S) { return S->result()->status; }

SolverLayout solver_layout(const DeviceSolver *S)
{
  return SolverLayout{S->plan.pos, S->plan.to_solver, S->plan.hold, S->Bp, (size_t)S->K * S->Bp};
}

SolverFactor solver_factor(const DeviceSolver *S)
{
  return SolverFactor{&S->host_plan, S->h_blocks(), S->h_X.data(), S->Bp, S->Bs, S->factor_damp, S->epoch, S->factor_valid};
}

// a candidate for a solution that is on the device already (the dogleg step's blends: window_dogleg.hip): solve_retract_kernel
// itself, so the candidate, its mirrors and |delta|^2 are what a solve with this solution leaves, in every bit.  The word
// the kernel waits for is given before the launch
int solver_retract_from(DeviceSolver *S, hipStream_t stream, const double *x_dev, const float *vars0, float *vars1, int CS)
{
  S->go_epoch = (S->go_epoch + 1) & 0x7fffffffu;
  if (S->go_epoch == 0)
    S->go_epoch = 1;
  std::atomic_thread_fence(std::memory_order_release);
  *const_cast<volatile unsigned *>(&S->result()->go) = S->go_epoch;
  hipLaunchKernelGGL(solve_retract_kernel, dim3(1), dim3(1024), 0, stream, x_dev, S->K, S->B, S->Bp, CS, S->VS, S->plan.pos,
                     S->plan.hold, S->plan.to_solver, vars0, vars1, S->host_vars(), S->host_delta(), S->result(), S->go_epoch);
  return (int)hipGetLastError();
}

} // namespace sage
