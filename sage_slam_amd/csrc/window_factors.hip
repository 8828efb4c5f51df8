// window_factors.hip -- f2: per-edge results and the per-Values factor cache behind the gtsam adapter
// (photometric_factor.cpp:72-219, geometric_factor.cpp:41-233): batched prepass, factor blocks, NearestPsd on host threads
// and on the device, for the dense factors and for the window's keypoint and graph terms alike: a cached factor is a
// FactorRef into a FactorSlot (window_state.h) with a FactorShape (factor_blocks.h).
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
// device-to-host copy of the per-edge and per-term results; every other factor is served from the host cache.
extern "C" int sage_window_prepass(SageWindow *w, const float *pose12, const float *codes, const float *scales,
                                   int jacobians, int *recomputed)
{
  if (!w || !w->finalized || !pose12 || !codes || !scales)
    return SAGE_E_INVALID;
  const int K = w->K, CS = w->cfg.CS;
  FactorCache &fc = w->fc;
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
  // SAGE_RELIN_STALE: the dense slots' host rows still mirror the device's per-edge results when no linearize has written
  // those since the last pull -- an error-only prepass at other values in between leaves both alone.  The stale-mode
  // linearize below then re-evaluates some edges, and only their rows are pulled
  const bool stale_mode = w->relin.mode == SAGE_RELIN_STALE;
  const bool rows_kept = stale_mode && jacobians && fc.rows_pulled && fc.rows_serial == w->dense_serial;
  if (jacobians)
  {
    if ((rc = sage_window_linearize(w)))
      return rc;
  }
  else if ((rc = sage_window_error(w, 0)))
    return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  auto pull = [](std::vector<float> &dst, const float *src, size_t n) -> hipError_t {
    dst.resize(n);
    return n ? hipMemcpy(dst.data(), src, n * sizeof(float), hipMemcpyDeviceToHost) : hipSuccess;
  };
  // rows `edges` (ascending) of a [n][width] array, a run of consecutive edges per copy
  auto pull_rows = [](std::vector<float> &dst, const float *src, size_t width, const std::vector<int32_t> &edges) -> hipError_t {
    for (size_t i = 0; i < edges.size();)
    {
      size_t j = i + 1;
      while (j < edges.size() && edges[j] == edges[j - 1] + 1)
        ++j;
      const size_t at = (size_t)edges[i] * width;
      const hipError_t e = hipMemcpy(dst.data() + at, src + at, (j - i) * width * sizeof(float), hipMemcpyDeviceToHost);
      if (e != hipSuccess)
        return e;
      i = j;
    }
    return hipSuccess;
  };
  if (jacobians)
    w->relin.counts.host_entries_pulled = 0;
  const TermSide &ts = w->terms;
  const bool with_terms = ts.n_stats() > 0;
  for (int sl = 0; sl < FactorCache::kSlots; ++sl)
  {
    // what slot sl caches: a dense factor type's per-edge results, or a term group's systems of a window that has terms
    const bool dense = sl < 2;
    const int g = sl - 2;
    if (!(dense ? (sl == kPhoto ? w->cfg.use_photo : w->cfg.use_geo) : with_terms))
      continue;
    if (jacobians)
    {
      FactorSlot &s = fc.slot[sl];
      const size_t n = dense ? ne : (size_t)ts.layout.count[g];
      s.D = dense ? dense_dim(sl, CS) : (size_t)TermResults::dim(g, CS);
      s.live = dense ? &w->dense[sl].AtA : &ts.AtA[g];
      s.live_serial = dense ? &w->dense_serial : &ts.serial;
      if (dense && rows_kept && s.A.size() == n * s.D * s.D && s.b.size() == n * s.D)
      {
        const std::vector<int32_t> &ev = w->relin.evaluated[sl];
        SAGE_HIP(pull_rows(s.A, s.live->as<float>(), s.D * s.D, ev));
        SAGE_HIP(pull_rows(s.b, w->dense[sl].Atb.as<float>(), s.D, ev));
        w->relin.counts.host_entries_pulled += (int32_t)ev.size();
      }
      else
      {
        SAGE_HIP(pull(s.A, s.live->as<float>(), n * s.D * s.D));
        SAGE_HIP(pull(s.b, dense ? w->dense[sl].Atb.as<float>() : ts.Atb[g].as<float>(), n * s.D));
        if (dense)
          w->relin.counts.host_entries_pulled += (int32_t)n;
      }
      s.serial = *s.live_serial;
    }
    if (dense) // the {error, inliers} this pass wrote: the linearization's half, or the error pass's
      SAGE_HIP(pull(fc.stats[sl], jacobians ? w->dense[sl].stats.as<float>() : w->dense[sl].error_stats(), ne * 2));
  }
  if (jacobians)
  {
    fc.rows_pulled = true;
    fc.rows_serial = w->dense_serial;
  }
  if (with_terms) // the {error, inliers} set this pass wrote
    SAGE_HIP(pull(fc.stats[2], ts.results(jacobians != 0).stats, (size_t)2 * ts.n_stats()));
  fc.lin = jacobians != 0;
  fc.err = true;
  if (recomputed)
    *recomputed = 1;
  return SAGE_OK;
}

// ---- a cached factor.  FactorRef: the entry of a slot it is cut from, where its {error, inliers} stand, its shape
struct FactorRef
{
  int slot, entry;    // entry < 0: a directed edge that is not one of this rank's dense edges
  int stat_set, stat; // FactorCache::stats[stat_set][2 * stat]
  FactorShape shape;
};
static FactorRef dense_ref(const SageWindow *w, int type, int local_edge)
{
  return FactorRef{type, local_edge, type, local_edge, dense_factor_shape(type, w->cfg.CS)};
}
// SAGE_OK and *ref, or SAGE_E_INVALID: no such term, or another rank's
static int term_ref(const SageWindow *w, bool graph, int term, FactorRef *ref)
{
  if (!w || !w->finalized)
    return SAGE_E_INVALID;
  const TermSide &ts = w->terms;
  if (term < 0 || term >= (graph ? (int)ts.gt_added.size() : (int)ts.kp_added.size()))
    return SAGE_E_INVALID;
  const plan::TermSlot &at = (graph ? ts.layout.graph : ts.layout.kp)[term];
  const int kind = graph ? ts.gt_added[term].kind : ts.kp_added[term].kind;
  *ref = FactorRef{2 + at.group, at.out, 2, at.stat, term_factor_shape(graph ? SAGE_TERM_GRAPH : SAGE_TERM_KEYPOINT, kind, w->cfg.CS)};
  return at.local < 0 || !ref->shape.nk ? SAGE_E_INVALID : SAGE_OK;
}

// every cached factor of this rank: the photometric and the geometric factors by local edge, the keypoint terms and the
// graph terms in launch order
static std::vector<FactorRef> local_refs(const SageWindow *w)
{
  std::vector<FactorRef> out;
  for (int type = kPhoto; type <= kGeo; ++type)
    for (size_t i = 0; i < w->fc.slot[type].n(); ++i)
      out.push_back(dense_ref(w, type, (int)i));
  FactorRef r;
  for (int id : w->terms.layout.kp_order)
    if (term_ref(w, false, id, &r) == SAGE_OK)
      out.push_back(r);
  for (int id : w->terms.layout.graph_order)
    if (term_ref(w, true, id, &r) == SAGE_OK)
      out.push_back(r);
  return out;
}

// the factor's own sub-matrix inside its entry of a slot's [n][D][D] array (a dense factor's: the entry)
template <class T>
static T *own_matrix(T *base, const FactorRef &r)
{
  const size_t D = (size_t)r.shape.D_group;
  return base + (size_t)r.entry * D * D + (size_t)r.shape.first * (D + 1);
}

// NearestPsd of the factor's own matrix, into its columns of the entry of the slot's C (`own`: scratch)
static int project_own(FactorSlot &sl, const FactorRef &r, int psd_mode, std::vector<double> &own)
{
  const size_t D = (size_t)r.shape.D_group, Do = (size_t)r.shape.D_own;
  own.resize(Do * Do);
  const int rc = factor_psd(r.shape, sl.A.data() + (size_t)r.entry * D * D, psd_mode, own.data());
  double *dst = own_matrix(sl.C.data(), r);
  for (size_t a = 0; a < Do && !rc; ++a)
    std::memcpy(dst + a * D, own.data() + a * Do, Do * sizeof(double));
  return rc;
}

// the factor from the cache: prepared for this psd_mode, so cut; otherwise project and cut.  `missing`: the status of a
// factor the cache has no entry for (a dense edge that is not local: SAGE_E_INVALID; a term: SAGE_E_STATE, a cache pulled
// before the window had its terms, which cannot happen after finalize)
static int cached_factor(const FactorCache &fc, const FactorRef &r, int missing, int psd_mode, double *G_out, double *g_out,
                         double *f_out, int32_t *dims_out, int32_t *nkeys_out)
{
  if (!fc.lin)
    return SAGE_E_STATE;
  const FactorSlot &sl = fc.slot[r.slot];
  const std::vector<float> &st = fc.stats[r.stat_set];
  const size_t D = (size_t)r.shape.D_group, e = (size_t)r.entry;
  if (r.entry < 0 || (e + 1) * D * D > sl.A.size() || (size_t)r.stat * 2 + 1 >= st.size())
    return missing;
  if (f_out)
    *f_out = (double)st[(size_t)r.stat * 2];
  const float *b = sl.b.data() + e * D;
  if (fc.psd_mode == psd_mode && (e + 1) * D * D <= sl.C.size()) // prepared already: cut the blocks from the factor's own columns
    return factor_cut(r.shape, own_matrix(sl.C.data(), r), (int)D, b, G_out, g_out, dims_out, nkeys_out);
  return factor_blocks(r.shape, sl.A.data() + e * D * D, b, psd_mode, G_out, g_out, dims_out, nkeys_out);
}

static int cached_error(const FactorCache &fc, const FactorRef &r, int missing, double *err_out)
{
  if (!fc.err)
    return SAGE_E_STATE;
  const std::vector<float> &st = fc.stats[r.stat_set];
  if (r.entry < 0 || (size_t)r.stat * 2 + 1 >= st.size())
    return missing;
  *err_out = (double)st[(size_t)r.stat * 2];
  return SAGE_OK;
}

extern "C" int sage_window_factor(const SageWindow *w, int type, int e, int psd_mode, double *G_out, double *g_out,
                                  double *f_out, int *dims_out, int *nkeys_out)
{
  if (!w || !w->finalized || (type != 0 && type != 1))
    return SAGE_E_INVALID;
  return cached_factor(w->fc, dense_ref(w, type, window_local_edge(w, e)), SAGE_E_INVALID, psd_mode, G_out, g_out, f_out,
                       dims_out, nkeys_out);
}
extern "C" int sage_window_factor_error(const SageWindow *w, int type, int e, double *err_out)
{
  if (!w || !w->finalized || (type != 0 && type != 1) || !err_out)
    return SAGE_E_INVALID;
  return cached_error(w->fc, dense_ref(w, type, window_local_edge(w, e)), SAGE_E_INVALID, err_out);
}

static int term_factor(const SageWindow *w, bool graph, int term, int psd_mode, double *G_out, double *g_out, double *f_out,
                       int32_t *dims_out, int32_t *nkeys_out)
{
  FactorRef r;
  if (term_ref(w, graph, term, &r) || psd_mode < 0 || psd_mode > 2 || !G_out || !g_out)
    return SAGE_E_INVALID;
  return cached_factor(w->fc, r, SAGE_E_STATE, psd_mode, G_out, g_out, f_out, dims_out, nkeys_out);
}
static int term_factor_error(const SageWindow *w, bool graph, int term, double *err_out)
{
  FactorRef r;
  if (term_ref(w, graph, term, &r) || !err_out)
    return SAGE_E_INVALID;
  return cached_error(w->fc, r, SAGE_E_STATE, err_out);
}

extern "C" int sage_window_keypoint_factor(const SageWindow *w, int term, int psd_mode, double *G_out, double *g_out,
                                           double *f_out, int32_t *dims_out, int32_t *nkeys_out)
{
  return term_factor(w, false, term, psd_mode, G_out, g_out, f_out, dims_out, nkeys_out);
}
extern "C" int sage_window_keypoint_factor_error(const SageWindow *w, int term, double *err_out)
{
  return term_factor_error(w, false, term, err_out);
}
extern "C" int sage_window_graph_factor(const SageWindow *w, int term, int psd_mode, double *G_out, double *g_out,
                                        double *f_out, int32_t *dims_out, int32_t *nkeys_out)
{
  return term_factor(w, true, term, psd_mode, G_out, g_out, f_out, dims_out, nkeys_out);
}
extern "C" int sage_window_graph_factor_error(const SageWindow *w, int term, double *err_out)
{
  return term_factor_error(w, true, term, err_out);
}

// NearestPsd of EVERY cached factor on `n_threads` host threads (0 = a quarter of the host's hardware threads, at most 64): the per-factor
// projection is the host cost of the gtsam path (an SVD / eigen-decomposition of a 45 x 45 and a 78 x 78 matrix per link
// direction, photometric_factor.cpp:142-149) -- ISAM2 pays it factor by factor, here it is paid once per Values in
// parallel and the reads only cut blocks afterwards.  Every factor is projected on its own D_own x D_own matrix
// (factor_psd's definition).
extern "C" int sage_window_prepare_factors(SageWindow *w, int psd_mode, int n_threads)
{
  if (!w || !w->finalized || psd_mode < 0 || psd_mode > 2)
    return SAGE_E_INVALID;
  FactorCache &fc = w->fc;
  if (!fc.lin)
    return SAGE_E_STATE;
  if (fc.psd_mode == psd_mode)
    return SAGE_OK;
  fc.psd_mode = -1; // the projected matrices are being rewritten: whatever they held is gone until this call succeeds
  for (FactorSlot &sl : fc.slot)
    sl.C.assign(sl.A.size(), 0.0);
  // the work queue, longest jobs first: the geometric factors and match-geometry terms (14 + 2 CS), the photometric factors
  // and reprojection terms (13 + CS), then the terms of 14, 12 and 1 columns
  std::vector<FactorRef> jobs = local_refs(w);
  std::stable_sort(jobs.begin(), jobs.end(), [](const FactorRef &a, const FactorRef &b) { return a.shape.D_own > b.shape.D_own; });
  const size_t total = jobs.size();
  if (n_threads <= 0)
    n_threads = (int)std::min<unsigned>(64u, std::max(1u, std::thread::hardware_concurrency() / 4)); // a quarter of the host, <= 64
  n_threads = (int)std::min<size_t>((size_t)n_threads, std::max<size_t>(1, total));
  std::atomic<size_t> next{0};
  std::atomic<int> bad{0};
  auto work = [&]() {
    std::vector<double> own;
    for (;;)
    {
      const size_t i = next.fetch_add(1, std::memory_order_relaxed);
      if (i >= total)
        return;
      const int rc = project_own(fc.slot[jobs[i].slot], jobs[i], psd_mode, own);
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
// slot that has entries, the projected matrices and their records copied back behind them, one wait.  The kernel reads the
// window's own per-edge AtA (a term group's AtA) while that still is the linearisation the cache was pulled from
// (FactorSlot::serial); after another linearize the cached copy is uploaded instead.  A term group is projected as it lies,
// at the group's D: a kind that owns fewer columns sits in exact zeros, which the sweeps skip and the acceptance test passes,
// and its blocks are cut from its own columns.  A factor whose record is not clean (sweep cap, non-finite input) is
// projected again on the host, so such inputs come out as sage_window_prepare_factors leaves them.
extern "C" int sage_window_prepare_factors_device(SageWindow *w, SagePsdStats *worst)
{
  if (!w || !w->finalized)
    return SAGE_E_INVALID;
  FactorCache &fc = w->fc;
  if (!fc.lin)
    return SAGE_E_STATE;
  fc.psd_launches = 0;
  if (fc.psd_mode == 1)
  {
    if (worst)
      *worst = fc.psd_worst;
    return SAGE_OK;
  }
  fc.psd_mode = -1; // (as above)
  std::vector<SagePsdStats> rec[FactorCache::kSlots];
  int rc;
  for (int i = 0; i < FactorCache::kSlots; ++i)
  {
    FactorSlot &sl = fc.slot[i];
    const size_t n = sl.n(), elems = sl.A.size();
    sl.C.resize(elems);
    rec[i].resize(n);
    if (!n)
      continue;
    const float *in = sl.live_AtA();
    if (!in)
    {
      if ((rc = sl.psd_in.reserve(elems * sizeof(float))))
        return rc;
      SAGE_HIP(hipMemcpyAsync(sl.psd_in.p, sl.A.data(), elems * sizeof(float), hipMemcpyHostToDevice, w->stream));
      in = sl.psd_in.as<float>();
    }
    if ((rc = sl.psd_out.reserve(elems * sizeof(double))) || (rc = sl.psd_stats.reserve(n * sizeof(SagePsdStats))))
      return rc;
    if ((rc = psd_project_enqueue(w->stream, (int)sl.D, (int)n, in, sl.psd_out.as<double>(), sl.psd_stats.as<SagePsdStats>())))
      return rc;
    ++fc.psd_launches;
  }
  for (int i = 0; i < FactorCache::kSlots; ++i)
    if (!rec[i].empty())
    {
      FactorSlot &sl = fc.slot[i];
      SAGE_HIP(hipMemcpyAsync(sl.C.data(), sl.psd_out.p, sl.C.size() * sizeof(double), hipMemcpyDeviceToHost, w->stream));
      SAGE_HIP(hipMemcpyAsync(rec[i].data(), sl.psd_stats.p, rec[i].size() * sizeof(SagePsdStats), hipMemcpyDeviceToHost, w->stream));
    }
  SAGE_HIP(hipStreamSynchronize(w->stream));
  // the worst record: the highest status, then the most sweeps, then the most bump rounds; a factor whose record is not
  // clean: the host's projection of its own matrix, into its columns of the entry
  SagePsdStats worst_rec{};
  bool any = false;
  std::vector<double> own;
  for (const FactorRef &r : local_refs(w))
  {
    if ((size_t)r.entry >= rec[r.slot].size())
      return SAGE_E_STATE;
    const SagePsdStats &s = rec[r.slot][r.entry];
    if (!any || s.status > worst_rec.status || (s.status == worst_rec.status && (s.sweeps > worst_rec.sweeps ||
        (s.sweeps == worst_rec.sweeps && s.bump_rounds > worst_rec.bump_rounds))))
      worst_rec = s;
    any = true;
    if (s.status != 0 && (rc = project_own(fc.slot[r.slot], r, 1, own)))
      return rc;
  }
  fc.psd_worst = worst_rec;
  if (worst)
    *worst = worst_rec;
  fc.psd_mode = 1;
  return SAGE_OK;
}

extern "C" int sage_window_prepare_factors_device_launches(const SageWindow *w) { return w ? w->fc.psd_launches : 0; }
