// window_prior.hip -- marginal priors on a window (PriorSide, window_state.h; layout and conventions: marginal.h): the third
// family of terms next to the keypoint and graph terms.  add / num / get, stage 7b of sage_window_finalize, the two kernels
// that run on every linearize (the first of them on every error pass too) with their launches, and sage_window_marginalize,
// which sums the factors incident to the dropped keyframes on the host and hands the sub-system to sage_schur_marginal.
//
// A prior's Lambda never passes through an fp32 result slot: finalize uploads its image in the packed layout and
// prior_add_kernel adds it to the assembled system, one writer per element, no atomics -- bit-reproducible from run to run.
#include "runtime_internal.h"

namespace sage
{

struct PriorEvalParams
{
  const marg::PriorTermDev *table;
  const double *lambda, *eta;
  const float *x0, *vars; // the linearisation points [m][VS] per term; the window's variable set [K][VS]
  int VS, CS;
  double *atb, *part; // of the pass
};

// grid (row tiles of 64, terms), one wave.  delta of the term in LDS (every tile rebuilds it: <= 16 pose_local and 16 * 33
// differences), then thread i forms (Lambda delta)_i as ONE serial fp64 sum over j ascending, reading Lambda[j][i] -- Lambda
// is symmetric, so this is the coalesced direction -- and the tile's partials of delta^T Lambda delta and eta^T delta are
// reduced in a fixed tree
__global__ __launch_bounds__(marg::kRowTile) void prior_eval_kernel(const PriorEvalParams p)
{
  __shared__ double s_delta[marg::kMaxKeyframes * 39];
  const marg::PriorTermDev &t = p.table[blockIdx.y];
  const int tile = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int m = t.m, n = t.n, CS = p.CS, B = 7 + CS;
  if (tile * marg::kRowTile >= n) // (the grid is the longest term's)
    return;
  const float *x0 = p.x0 + t.x0;
  if (tid < m)
  {
    double d6[6];
    pose_local(x0 + (size_t)tid * p.VS, p.vars + (size_t)t.kf[tid] * p.VS, d6);
    for (int i = 0; i < 6; ++i)
      s_delta[tid * B + i] = d6[i];
  }
  else
    for (int idx = tid - m; idx < m * (CS + 1); idx += marg::kRowTile - m) // code entries, then the scale: additive retraction
    {
      const int k = idx / (CS + 1), r = idx - k * (CS + 1);
      const int slot = r < CS ? 13 + r : 12;
      s_delta[k * B + 6 + r] = (double)p.vars[(size_t)t.kf[k] * p.VS + slot] - (double)x0[(size_t)k * p.VS + slot];
    }
  __syncthreads();
  const int i = tile * marg::kRowTile + tid;
  double quad = 0.0, lin = 0.0;
  if (i < n)
  {
    const double *L = p.lambda + t.lam;
    double acc = 0.0;
    // (the sum stays one chain in ascending j; kLoads of its loads are in flight at a time: a row of Lambda is n doubles
    //  away from the next, every load an L2 round trip -- with 8 in flight the kernel took 40 us at n = 312)
    constexpr int kLoads = 32;
    for (int j0 = 0; j0 < n; j0 += kLoads)
    {
      double v[kLoads];
#pragma unroll
      for (int u = 0; u < kLoads; ++u)
        v[u] = L[(size_t)(j0 + u < n ? j0 + u : n - 1) * n + i];
#pragma unroll
      for (int u = 0; u < kLoads; ++u)
        if (j0 + u < n)
          acc += v[u] * s_delta[j0 + u];
    }
    const double eta = p.eta[t.vec + i];
    p.atb[t.vec + i] = eta - acc;
    quad = s_delta[i] * acc;
    lin = eta * s_delta[i];
  }
  for (int off = 32; off > 0; off >>= 1)
  {
    quad += __shfl_down(quad, off);
    lin += __shfl_down(lin, off);
  }
  if (tid == 0)
  {
    p.part[2 * (t.tile0 + tile)] = quad;
    p.part[2 * (t.tile0 + tile) + 1] = lin;
  }
}

struct PriorAddParams
{
  const int32_t *image_blocks; // [n_blocks] packed block of each image entry
  const double *image;         // [n_blocks][B * B]
  const marg::PriorGradRow *grad;
  const int32_t *grad_start;   // [n_grad_kf + 1]
  const marg::PriorTermDev *table;
  const double *atb, *part;    // the linearize's
  double *packed, *tail_mirror;
  int n_blocks, n_grad_kf, n_terms, K, nlinks, B;
};

// behind the assembly, on its stream: workgroup per image block (packed block += image), per keyframe with prior rows (its
// gradient += the terms' Atb rows in term-id order), and one for the terms' errors, which ride in the geometric error slot of
// the tail as the graph terms' do
__global__ __launch_bounds__(256) void prior_add_kernel(const PriorAddParams p)
{
  const int bid = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int B = p.B, BB = B * B;
  double *g = p.packed + (size_t)(p.K + p.nlinks) * BB;
  if (bid < p.n_blocks)
  {
    double *dst = p.packed + (size_t)p.image_blocks[bid] * BB;
    const double *src = p.image + (size_t)bid * BB;
    for (int idx = tid; idx < BB; idx += (int)blockDim.x)
      dst[idx] += src[idx];
  }
  else if (bid < p.n_blocks + p.n_grad_kf)
  {
    const int a0 = p.grad_start[bid - p.n_blocks], a1 = p.grad_start[bid - p.n_blocks + 1];
    if (tid < B)
    {
      double *dst = g + (size_t)p.grad[a0].kf * B + tid;
      double acc = *dst;
      for (int a = a0; a < a1; ++a)
        acc += p.atb[p.grad[a].src + tid];
      *dst = acc;
    }
  }
  else if (tid == 0)
  {
    double *tail = g + (size_t)p.K * B; // [err_photo err_geo n_photo n_geo]
    const double e = tail[1] + marg::prior_error_total(p.table, p.n_terms, p.part);
    tail[1] = e;
    if (p.tail_mirror)
      p.tail_mirror[1] = e;
  }
}

} // namespace sage

// ---- add / num ------------------------------------------------------------------------------------------------------------
extern "C" int sage_window_add_prior_term(SageWindow *w, const SageMarginalPrior *prior, const int32_t *kf_map)
{
  if (!w || !prior || !kf_map)
    return SAGE_E_INVALID;
  if (w->finalized)
    return SAGE_E_STATE;
  if (prior->CS != w->cfg.CS)
    return SAGE_E_INVALID;
  if (const int rc = marg::check_keyframes(w->K, kf_map, prior->m)) // (the cap: the kernel's LDS and PriorTermDev::kf)
    return rc;
  for (const auto &ab : marg::missing_links(w->links, kf_map, prior->m))
  {
    const int rc = sage_window_add_keypoint_link(w, ab.first, ab.second); // structure only: a block of the packed system
    if (rc < 0)
      return rc;
  }
  w->priors.added.push_back(PriorSide::Added{*prior, std::vector<int32_t>(kf_map, kf_map + prior->m)});
  return (int)w->priors.added.size() - 1;
}

extern "C" int sage_window_num_prior_terms(const SageWindow *w) { return w ? (int)w->priors.added.size() : 0; }

// ---- stage 7b of sage_window_finalize: leaves this rank's prior terms on the device (every term on rank 0): table, Lambda /
//      eta / linearisation points, the image of the Lambda blocks, the gradient rows, room for both passes' Atb and partials ----
int finalize_priors(SageWindow *w)
{
  PriorSide &ps = w->priors;
  ps.layout = marg::PriorLayout();
  ps.h_table.clear();
  ps.n_tiles = ps.n_blocks = ps.n_grad_kf = 0;
  ps.evaluated = false;
  if (ps.added.empty())
    return SAGE_OK;
  const int B = w->B, VS = w->VS, CS = w->cfg.CS;
  std::vector<std::vector<int32_t>> maps;
  for (const PriorSide::Added &a : ps.added)
    maps.push_back(a.kf_map);
  ps.layout = marg::prior_layout(w->K, w->links, maps, w->rank);
  if (ps.layout.missing)
    return SAGE_E_STATE; // (add appends every pair's link)
  if (ps.n_local() == 0)
    return SAGE_OK;
  std::vector<double> lambda, eta;
  std::vector<float> x0;
  std::vector<const double *> lam_of(ps.added.size(), nullptr);
  std::vector<int> m_of(ps.added.size(), 0);
  std::vector<size_t> vec_of(ps.added.size(), 0);
  for (int id : ps.layout.local)
  {
    const SageMarginalPrior &p = ps.added[id].prior;
    marg::PriorTermDev t{};
    t.m = p.m;
    t.n = p.rows();
    for (int i = 0; i < p.m; ++i)
      t.kf[i] = ps.added[id].kf_map[i];
    t.tile0 = ps.n_tiles;
    ps.n_tiles += (t.n + marg::kRowTile - 1) / marg::kRowTile;
    t.lam = lambda.size();
    t.vec = eta.size();
    t.x0 = x0.size();
    t.c = p.c;
    lambda.insert(lambda.end(), p.Lambda.begin(), p.Lambda.end());
    eta.insert(eta.end(), p.eta.begin(), p.eta.end());
    x0.resize(x0.size() + (size_t)p.m * VS, 0.f);
    for (int i = 0; i < p.m; ++i) // a window's record: pose 12, scale, code CS
    {
      float *rec = &x0[t.x0 + (size_t)i * VS];
      std::copy_n(&p.pose[(size_t)i * 12], 12, rec);
      rec[12] = p.scale[i];
      std::copy_n(&p.code[(size_t)i * CS], CS, rec + 13);
    }
    lam_of[id] = p.Lambda.data();
    m_of[id] = p.m;
    vec_of[id] = t.vec;
    ps.h_table.push_back(t);
  }
  const std::vector<double> image = marg::prior_image(ps.layout, B, lam_of, m_of);
  std::vector<int32_t> blocks(ps.layout.blocks.begin(), ps.layout.blocks.end());
  std::vector<marg::PriorGradRow> grad;
  std::vector<int32_t> grad_start;
  for (const marg::GradEntry &ge : ps.layout.grad)
  {
    if (grad.empty() || grad.back().kf != ge.kf)
      grad_start.push_back((int32_t)grad.size());
    grad.push_back(marg::PriorGradRow{ge.kf, 0, vec_of[ge.term] + (size_t)ge.pos * B});
  }
  ps.n_grad_kf = (int)grad_start.size();
  grad_start.push_back((int32_t)grad.size());
  ps.n_blocks = (int)blocks.size();
  int rc;
  if ((rc = upload(ps.table, ps.h_table, w->stream)) || (rc = upload(ps.lambda, lambda, w->stream)) ||
      (rc = upload(ps.eta, eta, w->stream)) || (rc = upload(ps.x0, x0, w->stream)) || (rc = upload(ps.image, image, w->stream)) ||
      (rc = upload(ps.image_blocks, blocks, w->stream)) || (rc = upload(ps.grad, grad, w->stream)) ||
      (rc = upload(ps.grad_start, grad_start, w->stream)))
    return rc;
  for (int pass = 0; pass < 2; ++pass)
    if ((rc = ps.atb[pass].reserve(eta.size() * sizeof(double))) || (rc = ps.part[pass].reserve((size_t)2 * ps.n_tiles * sizeof(double))))
      return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream)); // (the host vectors go out of scope)
  return SAGE_OK;
}

// ---- the two launches (profiler slots 8 / 9) ----
template <class Launch>
static int timed_prior_launch(SageWindow *w, int slot, Launch launch)
{
  LaunchCommon lc{};
  prof_attach(w, slot, lc);
  if (lc.ev_start)
    (void)hipEventRecord(lc.ev_start, w->stream);
  launch();
  SAGE_HIP(hipGetLastError());
  if (lc.ev_stop)
    (void)hipEventRecord(lc.ev_stop, w->stream);
  return SAGE_OK;
}

int window_launch_prior_eval(SageWindow *w, int set, bool jac)
{
  PriorSide &ps = w->priors;
  if (ps.n_local() == 0)
    return SAGE_OK;
  const int pass = jac ? 0 : 1;
  int max_tiles = 1;
  for (const marg::PriorTermDev &t : ps.h_table)
    max_tiles = std::max(max_tiles, (t.n + marg::kRowTile - 1) / marg::kRowTile);
  const PriorEvalParams p{ps.table.as<marg::PriorTermDev>(), ps.lambda.as<double>(), ps.eta.as<double>(), ps.x0.as<float>(),
                          w->vars[set].as<float>(), w->VS, w->cfg.CS, ps.atb[pass].as<double>(), ps.part[pass].as<double>()};
  const int rc = timed_prior_launch(w, 8, [&] {
    hipLaunchKernelGGL(prior_eval_kernel, dim3(max_tiles, ps.n_local()), dim3(marg::kRowTile), 0, w->stream, p);
  });
  ps.evaluated |= jac && !rc;
  return rc;
}

int window_launch_prior_add(SageWindow *w, double *packed, double *tail_mirror)
{
  PriorSide &ps = w->priors;
  if (ps.n_local() == 0)
    return SAGE_OK;
  const PriorAddParams p{ps.image_blocks.as<int32_t>(), ps.image.as<double>(), ps.grad.as<marg::PriorGradRow>(),
                         ps.grad_start.as<int32_t>(), ps.table.as<marg::PriorTermDev>(), ps.atb[0].as<double>(),
                         ps.part[0].as<double>(), packed, tail_mirror, ps.n_blocks, ps.n_grad_kf, ps.n_local(), w->K,
                         (int)w->links.size(), w->B};
  return timed_prior_launch(w, 9, [&] {
    hipLaunchKernelGGL(prior_add_kernel, dim3(ps.n_blocks + ps.n_grad_kf + 1), dim3(256), 0, w->stream, p);
  });
}

const double *window_prior_partials(const SageWindow *w, bool jac, int *n_terms)
{
  *n_terms = w->priors.n_local();
  return *n_terms ? w->priors.part[jac ? 0 : 1].as<double>() : nullptr;
}

// ---- get: host copy of the last linearize of prior term `term`, in doubles ----
extern "C" int sage_window_get_prior_term(const SageWindow *w, int term, double *AtA, double *Atb, double *err)
{
  if (!w || term < 0 || term >= (int)w->priors.added.size())
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  const PriorSide &ps = w->priors;
  if (term >= ps.n_local())
    return SAGE_E_INVALID; // another rank's (local terms are the leading ids: all of them on rank 0)
  if (!ps.evaluated)
    return SAGE_E_STATE;
  const marg::PriorTermDev &t = ps.h_table[term];
  SAGE_HIP(hipStreamSynchronize(w->stream));
  if (AtA)
    SAGE_HIP(hipMemcpy(AtA, ps.lambda.as<double>() + t.lam, (size_t)t.n * t.n * sizeof(double), hipMemcpyDeviceToHost));
  if (Atb)
    SAGE_HIP(hipMemcpy(Atb, ps.atb[0].as<double>() + t.vec, (size_t)t.n * sizeof(double), hipMemcpyDeviceToHost));
  if (err)
  {
    std::vector<double> part((size_t)2 * ps.n_tiles);
    SAGE_HIP(hipMemcpy(part.data(), ps.part[0].p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    *err = marg::prior_term_error(t, part.data());
  }
  return SAGE_OK;
}

// ---- marginalize -------------------------------------------------------------------------------------------------------
namespace
{

// the sub-system over the keyframes in `pos` (>= 0: its block index), dense [n x n] with gradient and error
struct SubSystem
{
  int B, CS, n;
  const std::vector<int> &pos;
  std::vector<double> A, g;
  double e = 0.0;
  SubSystem(int B_, int CS_, int nkf, const std::vector<int> &pos_) : B(B_), CS(CS_), n(nkf * B_), pos(pos_), A((size_t)n * n, 0.0), g((size_t)n, 0.0) {}
  double &at(int ka, int r, int kb, int c) { return A[((size_t)pos[ka] * B + r) * n + (size_t)pos[kb] * B + c]; }
  // a keyframe's share of a per-edge system with column map `type`: its diagonal block and gradient rows (the assembly's
  // keyframe blocks)
  void add_diag(int type, const float *M, const float *b, int D, int kf, int role)
  {
    for (int bi = 0; bi < B; ++bi)
    {
      const int ci = marg::packed_col(type, role, bi, CS);
      if (ci < 0)
        continue;
      g[(size_t)pos[kf] * B + bi] += (double)b[ci];
      for (int bj = 0; bj < B; ++bj)
      {
        const int cj = marg::packed_col(type, role, bj, CS);
        if (cj >= 0)
          at(kf, bi, kf, bj) += (double)M[(size_t)ci * D + cj];
      }
    }
  }
  // ... and the link block of link (a, b), a < b, for the direction dir (0: a -> b): [row in a][column in b], mirrored
  void add_link(int type, const float *M, int D, int a, int b, int dir)
  {
    for (int bi = 0; bi < B; ++bi)
    {
      const int ci = marg::packed_col(type, dir, bi, CS);
      if (ci < 0)
        continue;
      for (int bj = 0; bj < B; ++bj)
      {
        const int cj = marg::packed_col(type, 1 - dir, bj, CS);
        if (cj < 0)
          continue;
        const double v = (double)M[(size_t)ci * D + cj];
        at(a, bi, b, bj) += v;
        at(b, bj, a, bi) += v;
      }
    }
  }
  // a whole per-edge system on directed edge 2 * link + dir
  void add_edge(int type, const float *M, const float *b, int D, int a, int bkf, int dir)
  {
    add_diag(type, M, b, D, dir == 0 ? a : bkf, 0);
    add_diag(type, M, b, D, dir == 0 ? bkf : a, 1);
    add_link(type, M, D, a, bkf, dir);
  }
};

template <class T>
int fetch(std::vector<T> &dst, const void *src, size_t n)
{
  dst.resize(n);
  return n ? (int)hipMemcpy(dst.data(), src, n * sizeof(T), hipMemcpyDeviceToHost) : 0;
}

} // namespace

// a keyframe's own diagonal priors as window_prior_error counts them at the current variables
static double keyframe_prior_error(const SageWindow *w, int k)
{
  const SageWindowConfig &c = w->cfg;
  double s = 0;
  for (int i = 0; i < c.CS; ++i)
    s += (double)w->hv.code[0][(size_t)k * c.CS + i] * w->hv.code[0][(size_t)k * c.CS + i];
  double e = c.code_prior_weight * s / c.CS;
  if (k == 0 && c.scale_prior_weight > 0)
  {
    const double d = std::log((double)w->hv.scale_init[0]) - std::log((double)w->hv.scale[0][0]);
    e += c.scale_prior_weight * d * d;
  }
  if (k == 0 && c.pose_prior_weight > 0)
  {
    double loc[6];
    sage::pose_local(&w->hv.pose[0][0], &w->hv.pose_init[0], loc);
    for (int i = 0; i < 6; ++i)
      e += c.pose_prior_weight * loc[i] * loc[i];
  }
  return e;
}

extern "C" int sage_window_marginalize(SageWindow *w, const int32_t *drop, int n_drop, SageMarginalPrior **out)
{
  if (!w || !drop || n_drop < 1 || !out)
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  if (w->world > 1)
    return SAGE_E_UNSUPPORTED; // (no rank holds every result)
  const int K = w->K, B = w->B, CS = w->cfg.CS;
  std::vector<char> is_drop(K, 0);
  for (int i = 0; i < n_drop; ++i)
  {
    if (drop[i] < 0 || drop[i] >= K || is_drop[drop[i]])
      return SAGE_E_INVALID;
    is_drop[drop[i]] = 1;
  }
  if (n_drop >= K)
    return SAGE_E_INVALID;
  // the per-edge and per-term results must be the linearisation at the current variables, and so must `packed`
  if (!w->have_lin || w->lin_epoch != w->vars_epoch || w->results_epoch != w->vars_epoch)
    return SAGE_E_STATE;
  const PriorSide &ps = w->priors;
  const TermSide &ts = w->terms;
  // the separator: every survivor that shares a link or a prior term with a dropped keyframe
  std::vector<char> in_sep(K, 0), prior_in(ps.added.size(), 0);
  for (const auto &l : w->links)
    if (is_drop[l.first] != is_drop[l.second])
      in_sep[is_drop[l.first] ? l.second : l.first] = 1;
  for (size_t t = 0; t < ps.added.size(); ++t)
  {
    for (int k : ps.added[t].kf_map)
      prior_in[t] |= is_drop[k];
    if (prior_in[t])
      for (int k : ps.added[t].kf_map)
        in_sep[k] = !is_drop[k];
  }
  std::vector<int> order, pos(K, -1); // the sub-system's keyframes: the dropped ones ascending, then the separator ascending
  for (int k = 0; k < K; ++k)
    if (is_drop[k])
      order.push_back(k);
  for (int k = 0; k < K; ++k)
    if (in_sep[k])
      order.push_back(k);
  const int m = (int)order.size() - n_drop;
  if (m < 1)
    return SAGE_E_INVALID; // (nothing the dropped keyframes could tell anybody)
  if (m > marg::kMaxKeyframes)
    return SAGE_E_UNSUPPORTED;
  for (size_t i = 0; i < order.size(); ++i)
    pos[order[i]] = (int)i;
  SubSystem sub(B, CS, (int)order.size(), pos);
  SAGE_HIP(hipStreamSynchronize(w->stream));

  // 1. the dense factors of the directed edges with a dropped end: the fp32 results of the last linearize, both factor types
  for (int type = 0; type < 2; ++type)
  {
    if (w->n_edges == 0 || !(type == kPhoto ? w->cfg.use_photo : w->cfg.use_geo))
      continue;
    const size_t D = dense_dim(type, CS);
    const EdgeOut eo = w->dense[type].out();
    std::vector<float> A, b, st;
    for (int e = 0; e < w->n_edges; ++e)
    {
      const int ge = w->local_edges[e], l = ge / 2;
      const int ka = w->links[l].first, kb = w->links[l].second;
      if (!is_drop[ka] && !is_drop[kb])
        continue;
      SAGE_HIP((hipError_t)fetch(A, eo.AtA + (size_t)e * D * D, D * D));
      SAGE_HIP((hipError_t)fetch(b, eo.Atb + (size_t)e * D, D));
      SAGE_HIP((hipError_t)fetch(st, eo.stats + (size_t)e * 2, 2));
      sub.add_edge(type, A.data(), b.data(), (int)D, ka, kb, ge % 2);
      sub.e += (double)st[0];
    }
  }
  // 2. the keypoint and graph terms on those edges, a scale-prior graph term on a dropped keyframe
  if (ts.n_stats() > 0)
  {
    if (!ts.linearized)
      return SAGE_E_STATE;
    const TermResults res = ts.results(true);
    auto add_term = [&](const plan::TermSlot &slot, int edge, int kf) -> int {
      const size_t D = (size_t)TermResults::dim(slot.group, CS);
      std::vector<float> A, b, st;
      SAGE_HIP((hipError_t)fetch(A, res.AtA(slot.group) + (size_t)slot.out * D * D, D * D));
      SAGE_HIP((hipError_t)fetch(b, res.Atb(slot.group) + (size_t)slot.out * D, D));
      SAGE_HIP((hipError_t)fetch(st, res.stats + (size_t)slot.stat * 2, 2));
      if (edge >= 0)
        sub.add_edge(slot.group, A.data(), b.data(), (int)D, w->links[edge / 2].first, w->links[edge / 2].second, edge % 2);
      else
        sub.add_diag(slot.group, A.data(), b.data(), (int)D, kf, 0);
      sub.e += (double)st[0];
      return SAGE_OK;
    };
    auto edge_dropped = [&](int edge) { return is_drop[w->links[edge / 2].first] || is_drop[w->links[edge / 2].second]; };
    int rc;
    for (size_t i = 0; i < ts.kp_added.size(); ++i)
      if (ts.layout.kp[i].local >= 0 && edge_dropped(ts.kp_added[i].edge) && (rc = add_term(ts.layout.kp[i], ts.kp_added[i].edge, -1)))
        return rc;
    for (size_t i = 0; i < ts.gt_added.size(); ++i)
    {
      const SageGraphTerm &t = ts.gt_added[i];
      if (ts.layout.graph[i].local < 0)
        continue;
      const bool unary = t.kind == SAGE_GRAPH_SCALE_PRIOR;
      if ((unary ? is_drop[t.kf] != 0 : edge_dropped(t.edge)) && (rc = add_term(ts.layout.graph[i], unary ? -1 : t.edge, t.kf)))
        return rc;
    }
  }
  // 3. the dropped keyframes' own diagonal priors
  {
    const sage::SolvePriors pri = window_solve_priors(w);
    for (int k = 0; k < K; ++k)
    {
      if (!is_drop[k])
        continue;
      for (int r = 0; r < B; ++r)
      {
        double da, ga;
        sage::prior_row(pri, k, r, CS, &w->hv.pose[0][(size_t)k * 12], w->hv.scale[0][k], &w->hv.code[0][(size_t)k * CS], da, ga,
                        w->hold.empty() ? 0 : w->hold[k]);
        sub.at(k, r, k, r) += da;
        sub.g[(size_t)pos[k] * B + r] += ga;
      }
      sub.e += keyframe_prior_error(w, k);
    }
  }
  // 4. every prior term that touches a dropped keyframe, whole: Lambda, its last Atb and error
  if (std::count(prior_in.begin(), prior_in.end(), 1) > 0)
  {
    if (!ps.evaluated)
      return SAGE_E_STATE;
    std::vector<double> part, atb;
    SAGE_HIP((hipError_t)fetch(part, ps.part[0].p, (size_t)2 * ps.n_tiles));
    for (size_t t = 0; t < ps.added.size(); ++t)
    {
      if (!prior_in[t])
        continue;
      const SageMarginalPrior &p = ps.added[t].prior;
      const std::vector<int32_t> &kf = ps.added[t].kf_map;
      const marg::PriorTermDev &td = ps.h_table[t];
      SAGE_HIP((hipError_t)fetch(atb, ps.atb[0].as<double>() + td.vec, (size_t)td.n));
      for (int i = 0; i < p.m; ++i)
        for (int r = 0; r < B; ++r)
        {
          sub.g[(size_t)pos[kf[i]] * B + r] += atb[(size_t)i * B + r];
          for (int j = 0; j < p.m; ++j)
            for (int c = 0; c < B; ++c)
              sub.at(kf[i], r, kf[j], c) += p.Lambda[((size_t)i * B + r) * td.n + (size_t)j * B + c];
        }
      sub.e += marg::prior_term_error(td, part.data());
    }
  }
  // 5. the hold rule (damped_system.h: hold_packed) before the elimination: a held row of a dropped keyframe is a row of the
  //    identity with a zero gradient and eliminates to nothing; a held row of a separator keyframe is a zero row of Lambda
  if (window_has_holds(w))
    for (int k : order)
      for (int r = 0; r < B; ++r)
      {
        if (!sage::row_held(w->hold[k], r, CS))
          continue;
        const size_t row = (size_t)pos[k] * B + r;
        for (int c = 0; c < sub.n; ++c)
          sub.A[row * sub.n + c] = sub.A[(size_t)c * sub.n + row] = 0.0;
        sub.A[row * sub.n + row] = is_drop[k] ? 1.0 : 0.0;
        sub.g[row] = 0.0;
      }
  // 6. the Schur complement onto the separator, linearised at the window's current variables
  const int nk = m * B;
  std::vector<int32_t> drop_rows((size_t)n_drop * B), ids(m);
  for (size_t i = 0; i < drop_rows.size(); ++i)
    drop_rows[i] = (int32_t)i;
  std::vector<double> Lambda((size_t)nk * nk), eta((size_t)nk);
  double c = 0.0;
  if (const int rc = sage_schur_marginal(sub.A.data(), sub.g.data(), sub.e, sub.n, drop_rows.data(), (int)drop_rows.size(),
                                         Lambda.data(), eta.data(), &c))
    return rc;
  std::vector<float> pose((size_t)m * 12), code((size_t)m * CS), scale(m);
  for (int i = 0; i < m; ++i)
  {
    const int k = order[n_drop + i];
    ids[i] = k;
    std::copy_n(&w->hv.pose[0][(size_t)k * 12], 12, &pose[(size_t)i * 12]);
    std::copy_n(&w->hv.code[0][(size_t)k * CS], CS, &code[(size_t)i * CS]);
    scale[i] = w->hv.scale[0][k];
  }
  return sage_marginal_prior_create(m, CS, Lambda.data(), eta.data(), c, pose.data(), code.data(), scale.data(), ids.data(), out);
}
