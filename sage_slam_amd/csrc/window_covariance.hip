// window_covariance.hip -- how certain a window's estimate is: the marginal covariances of the last solve (covariance.h's
// recursion on the factor the device solver left in host memory), kept on the host in keyframe ids and the window's row
// order, and the depth sigma maps the device forms from them (depth_sigma.hip).  Every entry point is opt-in: a window that
// never calls them launches and computes what it did without them.
//
// Sigma belongs to the linearization it was solved at.  A later solve overwrites the factor and so invalidates it; a later
// linearize or accept does not -- the caller reads the covariance of the step it has just taken.  At damping 0 Sigma is
// A^-1 of the whole system (dense factors, diagonal priors, keypoint, graph and prior terms): ISAM2::marginalCovariance for
// factors served with G = AtA.  With damping it is the inverse of the damped system.
#include "damped_system.h"
#include "runtime_internal.h"

// why the window cannot have a covariance at all, or SAGE_OK
int covariance_refusal(const SageWindow *w)
{
  if (!w->finalized)
    return SAGE_E_STATE;
  if (w->world > 1) // (no rank factorises the whole system: as sage_window_marginalize)
    return SAGE_E_UNSUPPORTED;
  if (w->dist.shard || !w->solver) // the domain-decomposed solve; the host solve of duplicate links: neither leaves this factor
    return SAGE_E_UNSUPPORTED;
  return SAGE_OK;
}

bool covariance_current(const SageWindow *w)
{
  return w->cov.valid && w->cov.epoch == solver_factor(w->solver).epoch;
}

extern "C" int sage_window_covariance(SageWindow *w, double *damp_out)
{
  if (!w)
    return SAGE_E_INVALID;
  if (const int rc = covariance_refusal(w))
    return rc;
  const SolverFactor f = solver_factor(w->solver);
  if (!w->have_lin || !f.valid) // no solve yet, a failed one, or the system has been dropped since
    return SAGE_E_STATE;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  CovarianceSide &cv = w->cov;
  const int K = w->K, B = w->B, CS = w->cfg.CS, Bs = f.Bs, nl = (int)w->links.size();
  if (!cv.planned)
  {
    cv.plan = cov::plan_covariance(*f.plan);
    cv.planned = true;
  }
  cv.valid = false;
  cv.work.resize((size_t)cv.plan.nblk * f.Bp * f.Bp);
  cov::selected_inverse(*f.plan, cv.plan, f.Bp, f.T, f.X, cv.work.data());
  // positions and solver rows -> keyframes and block rows; a held or dropped row has no variance
  cv.diag.assign((size_t)K * B * B, 0.0);
  cv.link.assign((size_t)nl * B * B, 0.0);
  std::vector<double> blk((size_t)Bs * Bs);
  auto place = [&](int a, int b, double *dst) {
    if (!cov::covariance_block(cv.plan, f.Bp, Bs, cv.work.data(), f.plan->pos[a], f.plan->pos[b], blk.data()))
      return false;
    const int ha = w->hold.empty() ? 0 : w->hold[a], hb = w->hold.empty() ? 0 : w->hold[b];
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c)
      {
        const int sr = w->rows.to_solver[r], sc = w->rows.to_solver[c];
        if (sr >= 0 && sc >= 0 && !sage::row_held(ha, r, CS) && !sage::row_held(hb, c, CS))
          dst[(size_t)r * B + c] = blk[(size_t)sr * Bs + sc];
      }
    return true;
  };
  for (int k = 0; k < K; ++k)
    if (!place(k, k, &cv.diag[(size_t)k * B * B]))
      return SAGE_E_STATE;
  for (int l = 0; l < nl; ++l)
    if (!place(w->links[l].first, w->links[l].second, &cv.link[(size_t)l * B * B]))
      return SAGE_E_STATE;
  cv.valid = true;
  cv.epoch = f.epoch;
  cv.damp = f.damp;
  if (damp_out)
    *damp_out = f.damp;
  return SAGE_OK;
}

extern "C" int sage_window_get_covariance(const SageWindow *w, int kf_a, int kf_b, double *Sigma)
{
  if (!w || !Sigma)
    return SAGE_E_INVALID;
  if (const int rc = covariance_refusal(w))
    return rc;
  if (kf_a < 0 || kf_a >= w->K || kf_b < 0 || kf_b >= w->K)
    return SAGE_E_INVALID;
  if (!covariance_current(w))
    return SAGE_E_STATE;
  const int B = w->B;
  if (kf_a == kf_b)
  {
    std::memcpy(Sigma, &w->cov.diag[(size_t)kf_a * B * B], sizeof(double) * B * B);
    return SAGE_OK;
  }
  const int l = marg::find_link(w->links, kf_a, kf_b);
  if (l < 0)
    return SAGE_E_INVALID;
  const double *S = &w->cov.link[(size_t)l * B * B];
  for (int r = 0; r < B; ++r)
    for (int c = 0; c < B; ++c)
      Sigma[(size_t)r * B + c] = kf_a < kf_b ? S[(size_t)r * B + c] : S[(size_t)c * B + r];
  return SAGE_OK;
}

// bias, basis, code and scale as the window's own depth items name them (window_build.hip): the planes of the keyframe's view
// -- its handle's, for a prepared keyframe -- and the current variable set on the device; S from the stored Sigma
DepthSigmaEntry window_sigma_entry(const SageWindow *w, int k, float *out)
{
  const float *vp = w->vars[0].as<float>() + (size_t)k * w->VS;
  const size_t B = (size_t)w->B;
  return DepthSigmaEntry{w->views[k].bias, w->views[k].basis, vp + 13, vp + 12, 0.f, &w->cov.diag[(size_t)k * B * B + 6 * B + 6], B, out};
}

// scripts/covariance_bench.py: the sigma kernel over all K keyframes and depth_batch_kernel over the window's depth items (the
// same bytes), alternating, `reps` times each between HIP events on the window's stream -> the medians in microseconds.
// Leaves the depth maps of the current variable set behind, as an error pass at set 0 would
extern "C" int sage_window_depth_sigma_timing(SageWindow *w, int mode, int reps, double *sigma_us, double *depth_batch_us)
{
  if (!w || reps < 1 || !sigma_us || !depth_batch_us || (mode != SAGE_DEPTH_VARIANCE && mode != SAGE_DEPTH_SIGMA))
    return SAGE_E_INVALID;
  if (const int rc = covariance_refusal(w))
    return rc;
  if (!covariance_current(w) || w->n_edges == 0)
    return SAGE_E_STATE;
  const int K = w->K, CS = w->cfg.CS, H = (int)w->cfg.pyr.cam[0].h, W = (int)w->cfg.pyr.cam[0].w;
  DevBuf out;
  if (const int rc = out.reserve((size_t)K * H * W * sizeof(float)))
    return rc;
  std::vector<DepthSigmaEntry> e(K);
  for (int k = 0; k < K; ++k)
    e[k] = window_sigma_entry(w, k, out.as<float>() + (size_t)k * H * W);
  struct Events
  {
    hipEvent_t a = nullptr, b = nullptr;
    ~Events()
    {
      if (a)
        (void)hipEventDestroy(a);
      if (b)
        (void)hipEventDestroy(b);
    }
  } ev;
  SAGE_HIP(hipEventCreate(&ev.a));
  SAGE_HIP(hipEventCreate(&ev.b));
  std::vector<float> ts, td;
  for (int i = 0; i < reps; ++i)
  {
    float ms = 0.f;
    SAGE_HIP(hipEventRecord(ev.a, w->stream));
    SAGE_HIP(launch_depth_batch(w->stream, CS, w->depth_items[0].as<DepthItem>(), w->n_depth, H, W, true, false));
    SAGE_HIP(hipEventRecord(ev.b, w->stream));
    SAGE_HIP(hipEventSynchronize(ev.b));
    SAGE_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
    td.push_back(ms);
    if (const int rc = depth_sigma_enqueue(w->stream, w->cov.stage, e.data(), K, H, W, CS, mode, ev.a, ev.b))
      return rc;
    SAGE_HIP(hipEventSynchronize(ev.b));
    SAGE_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
    ts.push_back(ms);
  }
  w->dpt_set = 0;
  w->dgrad_valid = false;
  relin_stamp_maps(w, 0, true, false);
  auto median_us = [](std::vector<float> &v) {
    std::sort(v.begin(), v.end());
    return 1e3 * (double)v[v.size() / 2];
  };
  *sigma_us = median_us(ts);
  *depth_batch_us = median_us(td);
  return SAGE_OK;
}

extern "C" int sage_window_depth_sigma(SageWindow *w, const int32_t *kfs, int n, int mode, float *const *out_dev)
{
  if (!w || !kfs || !out_dev || n < 1 || n > 65535 || (mode != SAGE_DEPTH_VARIANCE && mode != SAGE_DEPTH_SIGMA))
    return SAGE_E_INVALID;
  if (const int rc = covariance_refusal(w))
    return rc;
  const int K = w->K, CS = w->cfg.CS;
  for (int i = 0; i < n; ++i)
    if (kfs[i] < 0 || kfs[i] >= K || !out_dev[i])
      return SAGE_E_INVALID;
  if (!covariance_current(w))
    return SAGE_E_STATE;
  std::vector<DepthSigmaEntry> e(n);
  for (int i = 0; i < n; ++i)
    e[i] = window_sigma_entry(w, kfs[i], out_dev[i]);
  return depth_sigma_enqueue(w->stream, w->cov.stage, e.data(), n, (int)w->cfg.pyr.cam[0].h, (int)w->cfg.pyr.cam[0].w, CS, mode);
}
