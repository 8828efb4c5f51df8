// window_dogleg.hip -- Powell's dogleg on a finalized window (the optimiser the reference's ISAM2 runs: deepfactors.cpp:89,
// 397, 650, 1422).  One factorisation per iteration, at damping 0; every trial point of the iteration is a blend
// delta = a g + b n of the right-hand side and the Gauss-Newton point, so a rejected evaluation costs the candidate kernel
// and an error pass.  The kernels:
//   dogleg_fetch_kernel   n, the Gauss-Newton point, from the solve's pinned delta mirror into device memory (it survives
//                         the candidates that overwrite the mirror)
//   dogleg_block_kernel   one workgroup per diagonal / link block of the packed buffer: the block, read once, times g and
//                         times n (a link block also transposed) -> partial products, one slot per incidence entry
//   dogleg_reduce_kernel  one workgroup: per keyframe the partials in the order of its incidence list -> Ag, An; then the
//                         six dot products and |An - g|^2 in a fixed order -> pinned memory, behind a ticket
//   dogleg_blend_kernel   a g + b n in the solver's solution layout, on the device; the candidate is then made by
//                         solve_retract_kernel itself (solver_retract_from), so it is what a solve with that solution leaves
//                         in every bit.  (A second kernel around a shared retraction body was tried first: the compiler
//                         packs one of its fp32 multiplies differently there, so one multiply-add of the pose update is
//                         fused in one kernel and not in the other, and the poses differ in the last bit.)
// No floating-point atomics, none of these kernels waits on the host.  What an element of A and g is comes from
// damped_system.h at damping 0.  The policy and the dogleg point are host code without HIP (dogleg_host.cpp).
#include "damped_system.h"
#include "runtime_internal.h"

namespace sage
{

constexpr int kDoglegMaxB = 40; // rows of a keyframe's block (B = 7 + CS <= 39)

struct DoglegSystem
{
  const double *packed; // [K diag | nlinks link | g | 4 totals]
  const float *vars0;   // [K][VS] the current variables (the priors' gradients)
  const int32_t *hold;  // [K] masks of held variables, or null
  const int32_t *links; // [nlinks][2]
  const double *n;      // [K * B] the Gauss-Newton point
  double *g;            // [K * B] out: the right-hand side (written by the diagonal blocks' workgroups)
  double *part;         // [dogleg::partial_slots][2][B] out
  int K, nlinks, B, CS, VS;
  SolvePriors pri;
};

// g and n of keyframe kf into LDS, row r: the prior's gradient added, a held row exactly zero; *da: the prior's diagonal
__device__ inline void dogleg_load_row(const DoglegSystem &S, int kf, int hold, int r, double *s_g, double *s_n, double *da)
{
  const float *var = S.vars0 + (size_t)kf * S.VS; // pose 12, scale, code CS
  double d, ga;
  prior_row(S.pri, kf, r, S.CS, var, var[12], var + 13, d, ga, hold);
  const bool held = hold && row_held(hold, r, S.CS);
  const size_t at = (size_t)kf * S.B + r;
  const double *g = S.packed + (size_t)(S.K + S.nlinks) * S.B * S.B;
  s_g[r] = held ? 0.0 : damped_rhs_elem(g[at], ga);
  s_n[r] = held ? 0.0 : S.n[at];
  if (da)
    *da = d;
}

// Four waves.  A diagonal block: wave 0 forms its rows times g, wave 1 times n.  A link block (a, b), stored [row in a]
// [column in b]: waves 0 / 1 its rows times g_b / n_b (keyframe a's share), waves 2 / 3 its columns times g_a / n_a
// (keyframe b's).  Every lane sums its row or column front to back.
__global__ __launch_bounds__(256) void dogleg_block_kernel(const DoglegSystem S)
{
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int B = S.B, BB = B * B, blk = blockIdx.x;
  __shared__ double s_M[kDoglegMaxB * kDoglegMaxB];
  __shared__ double s_g[2][kDoglegMaxB], s_n[2][kDoglegMaxB], s_da[kDoglegMaxB];
  const double *src = S.packed + (size_t)blk * BB;
  if (blk < S.K)
  {
    const int hold = S.hold ? S.hold[blk] : 0;
    if (tid < B)
    {
      dogleg_load_row(S, blk, hold, tid, s_g[0], s_n[0], &s_da[tid]);
      S.g[(size_t)blk * B + tid] = s_g[0][tid];
    }
    for (int o = tid; o < BB; o += blockDim.x)
      s_M[o] = src[o];
    __syncthreads();
    if (wave < 2 && lane < B)
    {
      const int r = lane;
      const double *v = wave == 0 ? s_g[0] : s_n[0];
      const bool held_r = hold && row_held(hold, r, S.CS);
      double acc = 0.0;
      for (int c = 0; c < B; ++c)
      {
        const bool held = held_r || (hold && row_held(hold, c, S.CS));
        const double e = held ? held_diag_elem(r, c) : damped_diag_elem(s_M, B, r, c, s_da[r], 0.0);
        acc += e * v[c];
      }
      S.part[((size_t)dogleg::partial_slot(S.K, blk, 0) * 2 + wave) * B + r] = acc;
    }
    return;
  }
  const int l = blk - S.K, ka = S.links[2 * l], kb = S.links[2 * l + 1];
  const int ha = S.hold ? S.hold[ka] : 0, hb = S.hold ? S.hold[kb] : 0;
  if (wave < 2 && lane < B)
    dogleg_load_row(S, wave == 0 ? ka : kb, wave == 0 ? ha : hb, lane, s_g[wave], s_n[wave], nullptr);
  for (int o = tid; o < BB; o += blockDim.x)
  {
    const int r = o / B, c = o - r * B;
    const bool held = (ha | hb) && (row_held(ha, r, S.CS) || row_held(hb, c, S.CS));
    s_M[o] = held ? 0.0 : src[o];
  }
  __syncthreads();
  if (lane < B)
  {
    const bool transposed = wave >= 2;
    const double *v = transposed ? ((wave & 1) ? s_n[0] : s_g[0]) : ((wave & 1) ? s_n[1] : s_g[1]);
    double acc = 0.0;
    for (int j = 0; j < B; ++j)
      acc += s_M[link_elem(!transposed, lane, j, B)] * v[j];
    S.part[((size_t)dogleg::partial_slot(S.K, blk, transposed ? 1 : 0) * 2 + (wave & 1)) * B + lane] = acc;
  }
}

// per keyframe the partial products in list order -> Ag, An; the dots: every thread over its entries in ascending order,
// the lanes of a wave by the shuffle tree, the waves front to back
__global__ __launch_bounds__(1024) void dogleg_reduce_kernel(const double *__restrict__ part, const int32_t *__restrict__ offsets,
                                                             const int32_t *__restrict__ entries,
                                                             const double *__restrict__ g, const double *__restrict__ n,
                                                             double *__restrict__ Ag, double *__restrict__ An, int K, int B,
                                                             dogleg::HostRecord *rec, double epoch)
{
  constexpr int kSums = dogleg::kDots + 1;
  const int tid = threadIdx.x;
  double acc[kSums] = {0, 0, 0, 0, 0, 0, 0};
  for (int idx = tid; idx < K * B; idx += blockDim.x)
  {
    const int k = idx / B, r = idx - k * B;
    double ag = 0.0, an = 0.0;
    for (int e = offsets[k]; e < offsets[k + 1]; ++e)
    {
      const size_t at = (size_t)dogleg::partial_slot(K, entries[2 * e], entries[2 * e + 1]) * 2 * B + r;
      ag += part[at];
      an += part[at + B];
    }
    Ag[idx] = ag;
    An[idx] = an;
    const double gi = g[idx], ni = n[idx];
    acc[dogleg::kGG] += gi * gi;
    acc[dogleg::kGN] += gi * ni;
    acc[dogleg::kNN] += ni * ni;
    acc[dogleg::kGAG] += gi * ag;
    acc[dogleg::kGAN] += gi * an;
    acc[dogleg::kNAN] += ni * an;
    acc[dogleg::kDots] += (an - gi) * (an - gi);
  }
  __shared__ double s_w[16][kSums];
  for (int q = 0; q < kSums; ++q)
  {
    double v = acc[q];
    for (int off = 32; off > 0; off >>= 1)
      v += __shfl_down(v, off);
    if ((tid & 63) == 0)
      s_w[tid >> 6][q] = v;
  }
  __syncthreads();
  if (tid == 0)
  {
    for (int q = 0; q < kSums; ++q)
    {
      double tot = 0.0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w)
        tot += s_w[w][q];
      (q < dogleg::kDots ? rec->dots[q] : rec->resid2) = tot;
    }
    // the record is visible to the host before the ticket is
    __threadfence_system();
    *reinterpret_cast<volatile double *>(&rec->ticket) = epoch;
  }
}

// the solve's delta (pinned host memory, read over PCIe) -> n on the device
__global__ __launch_bounds__(256) void dogleg_fetch_kernel(const double *__restrict__ h_delta, double *__restrict__ n, int count)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count)
    n[i] = h_delta[i];
}

// x = a g + b n in the solver's layout (SolverLayout); the rows the retraction never reads -- held ones, the padding -- are
// left alone.  A pure Gauss-Newton point is b n itself, a pure steepest-descent point a g: no term of the other vector
__global__ __launch_bounds__(256) void dogleg_blend_kernel(const double *__restrict__ g, const double *__restrict__ n, double a,
                                                           double b, int K, int B, int CS, SolverLayout L, double *__restrict__ x)
{
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= K * B)
    return;
  const int k = idx / B, r = idx - k * B;
  if (L.hold && row_held(L.hold[k], r, CS))
    return;
  x[(size_t)L.pos[k] * L.Bp + L.to_solver[r]] = a == 0.0 ? b * n[idx] : (b == 0.0 ? a * g[idx] : a * g[idx] + b * n[idx]);
}

} // namespace sage

// ---- host side ----
static int dogleg_check(const SageWindow *w)
{
  if (!w)
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  // one rank that sums nothing, and the device solver (a window with duplicate links has none: sage_block_solve sums them)
  if (w->world > 1 || w->dist.allreduce || !w->solver)
    return SAGE_E_UNSUPPORTED;
  return SAGE_OK;
}

static double *dogleg_vec(const SageWindow *w, int which) // 0 g, 1 Ag, 2 n, 3 An
{
  return w->dogleg.vec.as<double>() + (size_t)which * w->K * w->B;
}

// tables, vectors, the blend's solution buffer and the pinned record, once per window
static int dogleg_prepare(SageWindow *w)
{
  DoglegSide &d = w->dogleg;
  if (d.ready)
    return SAGE_OK;
  const int K = w->K, nl = (int)w->links.size(), B = w->B;
  const std::vector<int32_t> lk = window_link_pairs(w);
  const size_t n_ent = (size_t)dogleg::partial_slots(K, nl);
  std::vector<int32_t> tab((size_t)K + 1 + 2 * n_ent + 2 * (size_t)nl);
  int rc;
  if ((rc = sage_dogleg_incidence(K, nl, lk.data(), tab.data(), tab.data() + K + 1)))
    return rc;
  std::copy(lk.begin(), lk.end(), tab.begin() + K + 1 + 2 * n_ent);
  if ((rc = upload(d.tables, tab, w->stream)) || (rc = d.part.reserve(n_ent * 2 * B * sizeof(double))) ||
      (rc = d.vec.reserve((size_t)4 * K * B * sizeof(double))) || (rc = d.host.reserve(sizeof(dogleg::HostRecord))) ||
      (rc = d.x.reserve(solver_layout(w->solver).x_count * sizeof(double))))
    return rc;
  SAGE_HIP(hipMemsetAsync(d.vec.p, 0, (size_t)4 * K * B * sizeof(double), w->stream));
  SAGE_HIP(hipMemsetAsync(d.x.p, 0, solver_layout(w->solver).x_count * sizeof(double), w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream)); // (the tables are on their way from a local)
  std::memset(d.host.p, 0, sizeof(dogleg::HostRecord));
  d.ready = true;
  return SAGE_OK;
}

// enqueue the two product kernels and wait for the dots' ticket
static int dogleg_products(SageWindow *w, double *dots)
{
  DoglegSide &d = w->dogleg;
  if (!w->have_lin || !d.solved0)
    return SAGE_E_STATE;
  int rc;
  if ((rc = dogleg_prepare(w)))
    return rc;
  const int K = w->K, nl = (int)w->links.size(), B = w->B, CS = w->cfg.CS;
  if (B > kDoglegMaxB)
    return SAGE_E_UNSUPPORTED;
  if (!d.products)
  {
    // the first call behind the solve: the pinned mirror still holds its delta (a candidate would have overwritten it, and
    // is possible only after this call)
    hipLaunchKernelGGL(dogleg_fetch_kernel, dim3((K * B + 255) / 256), dim3(256), 0, w->stream, solver_host_delta(w->solver),
                       dogleg_vec(w, 2), K * B);
    SAGE_HIP(hipGetLastError());
  }
  const int32_t *tab = d.tables.as<int32_t>();
  const size_t n_ent = (size_t)dogleg::partial_slots(K, nl);
  DoglegSystem S{};
  S.packed = w->packed.as<double>();
  S.vars0 = w->vars[0].as<float>();
  S.hold = solver_layout(w->solver).hold;
  S.links = tab + K + 1 + 2 * n_ent;
  S.n = dogleg_vec(w, 2);
  S.g = dogleg_vec(w, 0);
  S.part = d.part.as<double>();
  S.K = K; S.nlinks = nl; S.B = B; S.CS = CS; S.VS = w->VS;
  S.pri = window_solve_priors(w);
  d.epoch += 1;
  hipLaunchKernelGGL(dogleg_block_kernel, dim3(K + nl), dim3(256), 0, w->stream, S);
  SAGE_HIP(hipGetLastError());
  hipLaunchKernelGGL(dogleg_reduce_kernel, dim3(1), dim3(1024), 0, w->stream, S.part, tab, tab + K + 1, S.g, S.n,
                     dogleg_vec(w, 1), dogleg_vec(w, 3), K, B, d.host.as<dogleg::HostRecord>(), (double)d.epoch);
  SAGE_HIP(hipGetLastError());
  const dogleg::HostRecord *rec = d.host.as<dogleg::HostRecord>();
  const double want = (double)d.epoch;
  const bool seen = spin_until([&] {
    double v;
    __atomic_load(&rec->ticket, &v, __ATOMIC_ACQUIRE);
    return v == want;
  });
  if (!seen)
    SAGE_HIP(hipStreamSynchronize(w->stream));
  // the ticket is behind the solve's retraction: its mirrors are complete, taking them up needs no synchronise
  if ((rc = window_sync_candidate(w, true)))
    return rc;
  std::copy_n(rec->dots, (int)dogleg::kDots, dots);
  d.products = d.vectors = true;
  return SAGE_OK;
}

// enqueue the candidate for delta = a g + b n; like the solve, it rewrites variable set 1 and its mirrors
static int dogleg_candidate(SageWindow *w, double a, double b)
{
  if (!w->dogleg.products)
    return SAGE_E_STATE;
  int rc = window_sync_candidate(w); // an unconsumed earlier candidate
  if (rc && rc != SAGE_E_NOT_PSD)
    return rc;
  if (w->dpt_set == 1)
    w->dpt_set = -1; // the candidate set is rewritten
  const int n = w->K * w->B;
  hipLaunchKernelGGL(dogleg_blend_kernel, dim3((n + 255) / 256), dim3(256), 0, w->stream, dogleg_vec(w, 0), dogleg_vec(w, 2), a, b,
                     w->K, w->B, w->cfg.CS, solver_layout(w->solver), w->dogleg.x.as<double>());
  SAGE_HIP(hipGetLastError());
  // (every earlier retraction has been waited for above or by the products' ticket: none is left to misread the new word)
  if ((rc = solver_retract_from(w->solver, w->stream, w->dogleg.x.as<double>(), w->vars[0].as<float>(), w->vars[1].as<float>(),
                                w->cfg.CS)))
    return rc;
  window_phase_mark(w, 3);
  w->cand_pending = true;
  return SAGE_OK;
}

extern "C" int sage_window_dogleg_products(SageWindow *w, double *dots)
{
  if (!w || !dots)
    return SAGE_E_INVALID;
  const int rc = dogleg_check(w);
  return rc ? rc : dogleg_products(w, dots);
}

extern "C" int sage_window_dogleg_candidate(SageWindow *w, double a, double b)
{
  const int rc = dogleg_check(w);
  return rc ? rc : dogleg_candidate(w, a, b);
}

extern "C" int sage_window_get_dogleg_vectors(SageWindow *w, double *g, double *Ag, double *n, double *An)
{
  int rc = dogleg_check(w);
  if (rc)
    return rc;
  if (!w->dogleg.vectors)
    return SAGE_E_STATE;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  double *out[4] = {g, Ag, n, An};
  for (int i = 0; i < 4; ++i)
    if (out[i])
      SAGE_HIP(hipMemcpy(out[i], dogleg_vec(w, i), (size_t)w->K * w->B * sizeof(double), hipMemcpyDeviceToHost));
  return SAGE_OK;
}

// the evaluation sage_dogleg_iterate calls: the candidate kernel, then the classic error pass; waits for the pass's tickets
static int dogleg_eval(void *ctx, double a, double b, double *f_candidate)
{
  SageWindow *w = static_cast<SageWindow *>(ctx);
  int rc;
  if ((rc = dogleg_candidate(w, a, b)) || (rc = window_error_pass(w, 1, true)))
    return rc;
  return window_total_error(w, 0, f_candidate, window_wait_error_totals(w));
}

extern "C" int sage_window_dogleg_step(SageWindow *w, SageDoglegState *st, const SageDoglegConfig *cfg)
{
  if (!w || !st || !cfg)
    return SAGE_E_INVALID;
  int rc = dogleg_check(w);
  if (rc || (rc = dogleg_prepare(w)))
    return rc;
  window_phase_mark(w, 0);
  if ((rc = window_linearize_set(w, 0, nullptr, false, true)))
    return rc;
  window_phase_mark(w, 2);
  // the one factorisation of the iteration; a non-positive pivot is reported here, before anything has moved
  if ((rc = sage_window_solve(w, 0.0, nullptr)))
    return rc;
  double dots[dogleg::kDots], f_error;
  if ((rc = dogleg_products(w, dots)) || (rc = window_total_error(w, 1, &f_error, true))) // (the dots' ticket has been seen)
    return rc;
  SageDoglegState s = *st;
  if ((rc = sage_dogleg_iterate(cfg, dots, f_error, dogleg_eval, w, &s)))
    return rc;
  if (s.accepted && (rc = sage_window_accept(w)))
    return rc;
  s.solves += 1;
  *st = s;
  return SAGE_OK;
}

extern "C" int sage_window_dogleg_run(SageWindow *w, SageDoglegState *st, const SageDoglegConfig *cfg, int n, double *trace,
                                      int *done)
{
  if (!w || !st || !cfg || n < 0)
    return SAGE_E_INVALID;
  int i = 0, rc = SAGE_OK;
  for (; i < n; ++i)
  {
    if ((rc = sage_window_dogleg_step(w, st, cfg)))
      break;
    if (trace)
    {
      double *t = trace + 7 * (size_t)i;
      t[0] = st->error;
      t[1] = st->candidate_error;
      t[2] = (double)st->accepted;
      t[3] = st->delta;
      t[4] = st->rho;
      t[5] = (double)st->region;
      t[6] = (double)st->evals;
    }
  }
  if (done)
    *done = i;
  return rc;
}
