// window_factors.hip -- f2: per-edge results and the per-Values factor cache behind the gtsam adapter
// (photometric_factor.cpp:72-219, geometric_factor.cpp:41-233): batched prepass, factor blocks, NearestPsd on host threads.
#include "runtime_internal.h"

extern "C" int sage_window_get_edge(const SageWindow *w, int type, int e, float *AtA, float *Atb, float *err,
                                    float *n_in)
{
  if (!w || !w->finalized || (type != 0 && type != 1))
    return SAGE_E_INVALID;
  // e is the global directed-edge index: link e/2, direction e%2 ; map to the local index
  const int le = window_local_edge(w, e);
  if (le < 0)
    return SAGE_E_INVALID;
  const size_t D = dense_dim(type, w->cfg.CS);
  const EdgeOut out = w->dense[type].out();
  SAGE_HIP(hipStreamSynchronize(w->stream));
  if (AtA)
    SAGE_HIP(hipMemcpy(AtA, out.AtA + (size_t)le * D * D, D * D * sizeof(float), hipMemcpyDeviceToHost));
  if (Atb)
    SAGE_HIP(hipMemcpy(Atb, out.Atb + (size_t)le * D, D * sizeof(float), hipMemcpyDeviceToHost));
  float s2[2];
  SAGE_HIP(hipMemcpy(s2, out.stats + (size_t)le * 2, 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (err)
    *err = s2[0];
  if (n_in)
    *n_in = s2[1];
  return SAGE_OK;
}

// ------------------------------------------------------------------------------------------------
// f2: the batched per-Values prepass behind the gtsam factors.  ISAM2 asks every factor of the window for
// linearize(values) / error(values) one at a time with the SAME Values; the reference answers each with its own kernel
// launches, .item() syncs and a NearestPsd (photometric_factor.cpp:72-219, geometric_factor.cpp:41-233).  Here the first
// factor that sees new values triggers ONE sage_window_linearize (or sage_window_error) for the whole window and one
// device-to-host copy of the per-edge results; every other factor is served from the host cache.
static int local_edge_index(const SageWindow *w, int e) { return window_local_edge(w, e); }

extern "C" int sage_window_prepass(SageWindow *w, const float *pose12, const float *codes, const float *scales,
                                   int jacobians, int *recomputed)
{
  if (!w || !w->finalized || !pose12 || !codes || !scales)
    return SAGE_E_INVALID;
  const int K = w->K, CS = w->cfg.CS;
  SageWindow::FactorCache &fc = w->fc;
  const size_t np = (size_t)K * 12, nc = (size_t)K * CS;
  const bool same = fc.pose.size() == np && std::memcmp(fc.pose.data(), pose12, np * sizeof(float)) == 0 &&
                    std::memcmp(fc.code.data(), codes, nc * sizeof(float)) == 0 &&
                    std::memcmp(fc.scale.data(), scales, (size_t)K * sizeof(float)) == 0;
  if (recomputed)
    *recomputed = 0;
  if (same && (fc.lin || (!jacobians && fc.err)))
    return SAGE_OK; // a cached linearisation also carries the errors (a1 returns the same error as a2)
  int rc;
  if (!same)
  {
    (void)window_sync_candidate(w);
    fc.lin = fc.err = false;
    fc.psd_mode = -1;
    fc.pose.assign(pose12, pose12 + np);
    fc.code.assign(codes, codes + nc);
    fc.scale.assign(scales, scales + K);
  }
  // the window's CURRENT variables become the requested values (both sets: a later solve starts from them)
  if (std::memcmp(w->hv.pose[0].data(), pose12, np * sizeof(float)) != 0 ||
      std::memcmp(w->hv.code[0].data(), codes, nc * sizeof(float)) != 0 ||
      std::memcmp(w->hv.scale[0].data(), scales, (size_t)K * sizeof(float)) != 0)
  {
    (void)window_sync_candidate(w);
    for (int s = 0; s < 2; ++s)
    {
      w->hv.pose[s].assign(pose12, pose12 + np);
      w->hv.code[s].assign(codes, codes + nc);
      w->hv.scale[s].assign(scales, scales + K);
    }
    if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
      return rc;
    w->have_lin = false;
  }
  const size_t ne = (size_t)w->n_edges;
  if (jacobians)
  {
    if ((rc = sage_window_linearize(w)))
      return rc;
  }
  else if ((rc = sage_window_error(w, 0)))
    return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  auto pull = [&](std::vector<float> &dst, const DevBuf &src, size_t n) -> hipError_t {
    dst.resize(n);
    return n ? hipMemcpy(dst.data(), src.p, n * sizeof(float), hipMemcpyDeviceToHost) : hipSuccess;
  };
  for (int type = kPhoto; type <= kGeo; ++type)
  {
    if (!(type == kPhoto ? w->cfg.use_photo : w->cfg.use_geo))
      continue;
    const size_t D = dense_dim(type, CS);
    if (jacobians)
    {
      SAGE_HIP(pull(fc.side[type].A, w->dense[type].AtA, ne * D * D));
      SAGE_HIP(pull(fc.side[type].b, w->dense[type].Atb, ne * D));
    }
    SAGE_HIP(pull(fc.side[type].s, w->dense[type].stats, ne * 2));
  }
  if (jacobians)
    fc.dense_serial = w->dense_serial;
  fc.lin = jacobians != 0;
  fc.err = true;
  if (recomputed)
    *recomputed = 1;
  return SAGE_OK;
}

extern "C" int sage_window_factor_error(const SageWindow *w, int type, int e, double *err_out)
{
  if (!w || !w->finalized || (type != 0 && type != 1) || !err_out)
    return SAGE_E_INVALID;
  const SageWindow::FactorCache &fc = w->fc;
  if (!fc.err)
    return SAGE_E_STATE;
  const int le = local_edge_index(w, e);
  const std::vector<float> &st = fc.side[type].s;
  if (le < 0 || (size_t)le * 2 + 1 >= st.size())
    return SAGE_E_INVALID;
  *err_out = (double)st[(size_t)le * 2];
  return SAGE_OK;
}

extern "C" int sage_window_factor(const SageWindow *w, int type, int e, int psd_mode, double *G_out, double *g_out,
                                  double *f_out, int *dims_out, int *nkeys_out)
{
  if (!w || !w->finalized || (type != 0 && type != 1))
    return SAGE_E_INVALID;
  const SageWindow::FactorCache &fc = w->fc;
  if (!fc.lin)
    return SAGE_E_STATE;
  const int le = local_edge_index(w, e);
  const int CS = w->cfg.CS;
  const size_t D = dense_dim(type, CS);
  const std::vector<float> &A = fc.side[type].A, &b = fc.side[type].b, &st = fc.side[type].s;
  if (le < 0 || ((size_t)le + 1) * D * D > A.size())
    return SAGE_E_INVALID;
  if (f_out)
    *f_out = (double)st[(size_t)le * 2];
  const std::vector<double> &Cc = fc.side[type].C;
  if (fc.psd_mode == psd_mode && ((size_t)le + 1) * D * D <= Cc.size()) // prepared on the host threads already
    return sage_factor_cut_blocks(type, CS, Cc.data() + (size_t)le * D * D, b.data() + (size_t)le * D, G_out, g_out,
                                  dims_out, nkeys_out);
  return sage_factor_hessian_blocks(type, CS, A.data() + (size_t)le * D * D, b.data() + (size_t)le * D, psd_mode, G_out,
                                    g_out, dims_out, nkeys_out);
}

// NearestPsd of EVERY cached factor on `n_threads` host threads (0 = a quarter of the host's hardware threads, at most 64): the per-factor
// projection is the host cost of the gtsam path (an SVD / eigen-decomposition of a 45 x 45 and a 78 x 78 matrix per link
// direction, photometric_factor.cpp:142-149) -- ISAM2 pays it factor by factor, here it is paid once per Values in
// parallel and sage_window_factor only cuts blocks afterwards.
extern "C" int sage_window_prepare_factors(SageWindow *w, int psd_mode, int n_threads)
{
  if (!w || !w->finalized || psd_mode < 0 || psd_mode > 2)
    return SAGE_E_INVALID;
  SageWindow::FactorCache &fc = w->fc;
  if (!fc.lin)
    return SAGE_E_STATE;
  if (fc.psd_mode == psd_mode)
    return SAGE_OK;
  const int CS = w->cfg.CS;
  const size_t Dp = dense_dim(kPhoto, CS), Dg = dense_dim(kGeo, CS);
  const size_t nep = fc.side[kPhoto].A.size() / (Dp * Dp), neg = fc.side[kGeo].A.size() / (Dg * Dg);
  fc.psd_mode = -1; // the projected matrices are being rewritten: whatever they held is gone until this call succeeds
  fc.side[kPhoto].C.assign(nep * Dp * Dp, 0.0);
  fc.side[kGeo].C.assign(neg * Dg * Dg, 0.0);
  const size_t total = nep + neg;
  if (n_threads <= 0)
    n_threads = (int)std::min<unsigned>(64u, std::max(1u, std::thread::hardware_concurrency() / 4)); // a quarter of the host, <= 64
  n_threads = (int)std::min<size_t>((size_t)n_threads, std::max<size_t>(1, total));
  std::atomic<size_t> next{0};
  std::atomic<int> bad{0};
  auto work = [&]() {
    for (;;)
    {
      // geometric factors first: they are the long jobs (78 x 78)
      const size_t i = next.fetch_add(1, std::memory_order_relaxed);
      if (i >= total)
        return;
      int rc;
      if (i < neg)
        rc = sage_factor_psd(1, CS, fc.side[kGeo].A.data() + i * Dg * Dg, psd_mode, fc.side[kGeo].C.data() + i * Dg * Dg);
      else
        rc = sage_factor_psd(0, CS, fc.side[kPhoto].A.data() + (i - neg) * Dp * Dp, psd_mode, fc.side[kPhoto].C.data() + (i - neg) * Dp * Dp);
      if (rc)
        bad.store(rc, std::memory_order_relaxed);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < n_threads; ++t)
    th.emplace_back(work);
  work();
  for (auto &t : th)
    t.join();
  if (bad.load())
    return bad.load();
  fc.psd_mode = psd_mode;
  return SAGE_OK;
}

// The same preparation on the device, psd_mode 1 only: one launch of the batched Higham projection (psd_project.hip) per
// factor type present, the projected matrices and their records copied back behind them, one wait.  The kernel reads the
// window's own per-edge AtA while that still is the linearisation the cache was pulled from (dense_serial); after another
// linearize the cached copy is uploaded instead.  A factor whose record is not clean (sweep cap, non-finite input) is
// projected again on the host, so such inputs come out as sage_window_prepare_factors leaves them.
extern "C" int sage_window_prepare_factors_device(SageWindow *w, SagePsdStats *worst)
{
  if (!w || !w->finalized)
    return SAGE_E_INVALID;
  SageWindow::FactorCache &fc = w->fc;
  if (!fc.lin)
    return SAGE_E_STATE;
  w->psd_launches = 0;
  if (fc.psd_mode == 1)
  {
    if (worst)
      *worst = w->psd_worst;
    return SAGE_OK;
  }
  const int CS = w->cfg.CS;
  fc.psd_mode = -1; // (as above)
  const bool fresh = fc.dense_serial == w->dense_serial;
  size_t D[2], ne[2];
  std::vector<SagePsdStats> rec[2];
  int rc;
  for (int type = kPhoto; type <= kGeo; ++type)
  {
    D[type] = dense_dim(type, CS);
    ne[type] = fc.side[type].A.size() / (D[type] * D[type]);
    fc.side[type].C.resize(ne[type] * D[type] * D[type]);
    rec[type].resize(ne[type]);
    if (!ne[type])
      continue;
    const size_t elems = ne[type] * D[type] * D[type];
    const float *in = w->dense[type].AtA.as<float>();
    if (!fresh)
    {
      if ((rc = w->psd_in[type].reserve(elems * sizeof(float))))
        return rc;
      SAGE_HIP(hipMemcpyAsync(w->psd_in[type].p, fc.side[type].A.data(), elems * sizeof(float), hipMemcpyHostToDevice, w->stream));
      in = w->psd_in[type].as<float>();
    }
    if ((rc = w->psd_out[type].reserve(elems * sizeof(double))) || (rc = w->psd_stats[type].reserve(ne[type] * sizeof(SagePsdStats))))
      return rc;
    if ((rc = psd_project_enqueue(w->stream, (int)D[type], (int)ne[type], in, w->psd_out[type].as<double>(),
                                  w->psd_stats[type].as<SagePsdStats>())))
      return rc;
    ++w->psd_launches;
  }
  for (int type = kPhoto; type <= kGeo; ++type)
    if (ne[type])
    {
      SAGE_HIP(hipMemcpyAsync(fc.side[type].C.data(), w->psd_out[type].p, fc.side[type].C.size() * sizeof(double),
                              hipMemcpyDeviceToHost, w->stream));
      SAGE_HIP(hipMemcpyAsync(rec[type].data(), w->psd_stats[type].p, ne[type] * sizeof(SagePsdStats), hipMemcpyDeviceToHost,
                              w->stream));
    }
  SAGE_HIP(hipStreamSynchronize(w->stream));
  SagePsdStats worst_rec{};
  bool any = false;
  for (int type = kPhoto; type <= kGeo; ++type)
    for (size_t i = 0; i < ne[type]; ++i)
    {
      const SagePsdStats &r = rec[type][i];
      // the worst record: the highest status, then the most sweeps, then the most bump rounds
      if (!any || r.status > worst_rec.status || (r.status == worst_rec.status && (r.sweeps > worst_rec.sweeps ||
          (r.sweeps == worst_rec.sweeps && r.bump_rounds > worst_rec.bump_rounds))))
        worst_rec = r;
      any = true;
      if (r.status != 0 && (rc = sage_factor_psd(type, CS, fc.side[type].A.data() + i * D[type] * D[type], 1,
                                                 fc.side[type].C.data() + i * D[type] * D[type])))
        return rc;
    }
  w->psd_worst = worst_rec;
  if (worst)
    *worst = worst_rec;
  fc.psd_mode = 1;
  return SAGE_OK;
}

extern "C" int sage_window_prepare_factors_device_launches(const SageWindow *w) { return w ? w->psd_launches : 0; }
