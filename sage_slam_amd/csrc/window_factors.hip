// window_factors.hip -- f2: per-edge results and the per-Values factor cache behind the gtsam adapter
// (photometric_factor.cpp:72-219, geometric_factor.cpp:41-233): batched prepass, factor blocks, NearestPsd on host threads
// and on the device; the same for the window's keypoint and graph terms (sage_window_keypoint_factor, sage_window_graph_factor).
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
  // the terms of a window that has some: every group's systems, and the {error, inliers} set this pass wrote
  const TermSide &ts = w->terms;
  if (ts.n_stats() > 0)
  {
    for (int g = 0; g < plan::kTermGroups && jacobians; ++g)
    {
      const size_t n = (size_t)ts.layout.count[g], D = (size_t)TermResults::dim(g, CS);
      SAGE_HIP(pull(fc.term[g].A, ts.AtA[g], n * D * D));
      SAGE_HIP(pull(fc.term[g].b, ts.Atb[g], n * D));
    }
    const size_t nst = (size_t)2 * ts.n_stats();
    fc.term_s.resize(nst);
    SAGE_HIP(hipMemcpy(fc.term_s.data(), ts.results(jacobians != 0).stats, nst * sizeof(float), hipMemcpyDeviceToHost));
    if (jacobians)
      fc.term_serial = ts.serial;
  }
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

// ---- a term's factor from the cache.  TermRef: where a term of this rank lives and what shape its factor has
struct TermRef
{
  int family, kind;
  plan::TermSlot slot;
  TermShape shape;
};
// SAGE_OK and *ref, or SAGE_E_INVALID: no such term, or another rank's
static int term_ref(const SageWindow *w, bool graph, int term, TermRef *ref)
{
  if (!w || !w->finalized)
    return SAGE_E_INVALID;
  const TermSide &ts = w->terms;
  if (term < 0 || term >= (graph ? (int)ts.gt_added.size() : (int)ts.kp_added.size()))
    return SAGE_E_INVALID;
  ref->family = graph ? SAGE_TERM_GRAPH : SAGE_TERM_KEYPOINT;
  ref->kind = graph ? ts.gt_added[term].kind : ts.kp_added[term].kind;
  ref->slot = (graph ? ts.layout.graph : ts.layout.kp)[term];
  ref->shape = term_shape(ref->family, ref->kind, w->cfg.CS);
  return ref->slot.local < 0 || !ref->shape.nk ? SAGE_E_INVALID : SAGE_OK;
}

// every term of this rank, keypoint terms then graph terms, each family in launch order
static std::vector<TermRef> local_terms(const SageWindow *w)
{
  std::vector<TermRef> out;
  TermRef r;
  for (int id : w->terms.layout.kp_order)
    if (term_ref(w, false, id, &r) == SAGE_OK)
      out.push_back(r);
  for (int id : w->terms.layout.graph_order)
    if (term_ref(w, true, id, &r) == SAGE_OK)
      out.push_back(r);
  return out;
}

// the term's own sub-matrix inside entry `out` of a group's [count][D][D] array
template <class T>
static T *term_own(T *base, const TermRef &r)
{
  const size_t D = (size_t)r.shape.D_group;
  return base + (size_t)r.slot.out * D * D + (size_t)r.shape.first * (D + 1);
}

static int term_factor(const SageWindow *w, bool graph, int term, int psd_mode, double *G_out, double *g_out, double *f_out,
                       int32_t *dims_out, int32_t *nkeys_out)
{
  TermRef r;
  if (term_ref(w, graph, term, &r) || psd_mode < 0 || psd_mode > 2 || !G_out || !g_out)
    return SAGE_E_INVALID;
  const SageWindow::FactorCache &fc = w->fc;
  if (!fc.lin)
    return SAGE_E_STATE;
  const SageWindow::FactorCache::TermGroup &tg = fc.term[r.slot.group];
  const size_t D = (size_t)r.shape.D_group, out = (size_t)r.slot.out;
  if ((out + 1) * D * D > tg.A.size() || (size_t)r.slot.stat * 2 + 1 >= fc.term_s.size())
    return SAGE_E_STATE; // (a cache pulled before the window had its terms: cannot happen after finalize)
  if (f_out)
    *f_out = (double)fc.term_s[(size_t)r.slot.stat * 2];
  const float *b = tg.b.data() + out * D;
  if (fc.psd_mode == psd_mode && (out + 1) * D * D <= tg.C.size()) // prepared already: cut the kind's blocks from its own columns
    return term_factor_cut(r.family, r.kind, w->cfg.CS, term_own(tg.C.data(), r), (int)D, b, G_out, g_out, dims_out, nkeys_out);
  return sage_term_factor_blocks(r.family, r.kind, w->cfg.CS, tg.A.data() + out * D * D, b, psd_mode, G_out, g_out, dims_out,
                                 nkeys_out);
}

static int term_factor_error(const SageWindow *w, bool graph, int term, double *err_out)
{
  TermRef r;
  if (term_ref(w, graph, term, &r) || !err_out)
    return SAGE_E_INVALID;
  const SageWindow::FactorCache &fc = w->fc;
  if (!fc.err || (size_t)r.slot.stat * 2 + 1 >= fc.term_s.size())
    return SAGE_E_STATE;
  *err_out = (double)fc.term_s[(size_t)r.slot.stat * 2];
  return SAGE_OK;
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
// parallel and sage_window_factor only cuts blocks afterwards.  The window's terms join the same queue, each with its own
// D_own x D_own matrix (sage_term_factor_blocks' definition).
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
  // the work queue, longest jobs first: the geometric factors and match-geometry terms (14 + 2 CS), the photometric factors
  // and reprojection terms (13 + CS), then the terms of 14, 12 and 1 columns; a term is projected on its own sub-matrix
  struct Job
  {
    int D, type; // type: the dense factor type, or -1: terms[index]
    size_t index;
  };
  const std::vector<TermRef> terms = fc.lin && w->terms.n_stats() > 0 ? local_terms(w) : std::vector<TermRef>();
  for (int g = 0; g < plan::kTermGroups; ++g)
    fc.term[g].C.assign(fc.term[g].A.size(), 0.0);
  std::vector<Job> jobs;
  for (size_t i = 0; i < neg; ++i)
    jobs.push_back({(int)Dg, kGeo, i});
  for (size_t i = 0; i < nep; ++i)
    jobs.push_back({(int)Dp, kPhoto, i});
  for (size_t i = 0; i < terms.size(); ++i)
    jobs.push_back({terms[i].shape.D_own, -1, i});
  std::stable_sort(jobs.begin(), jobs.end(), [](const Job &a, const Job &b) { return a.D > b.D; });
  const size_t total = jobs.size();
  if (n_threads <= 0)
    n_threads = (int)std::min<unsigned>(64u, std::max(1u, std::thread::hardware_concurrency() / 4)); // a quarter of the host, <= 64
  n_threads = (int)std::min<size_t>((size_t)n_threads, std::max<size_t>(1, total));
  std::atomic<size_t> next{0};
  std::atomic<int> bad{0};
  auto work = [&]() {
    std::vector<double> own; // a term's projected own matrix, before it goes into its columns of the group's entry
    for (;;)
    {
      const size_t i = next.fetch_add(1, std::memory_order_relaxed);
      if (i >= total)
        return;
      const Job &j = jobs[i];
      int rc;
      if (j.type >= 0)
      {
        const size_t DD = (size_t)j.D * j.D;
        rc = sage_factor_psd(j.type, CS, fc.side[j.type].A.data() + j.index * DD, psd_mode, fc.side[j.type].C.data() + j.index * DD);
      }
      else
      {
        const TermRef &r = terms[j.index];
        SageWindow::FactorCache::TermGroup &tg = fc.term[r.slot.group];
        const size_t D = (size_t)r.shape.D_group, Do = (size_t)r.shape.D_own;
        own.resize(Do * Do);
        rc = term_factor_psd(r.family, r.kind, CS, tg.A.data() + (size_t)r.slot.out * D * D, psd_mode, own.data());
        double *dst = term_own(tg.C.data(), r);
        for (size_t a = 0; a < Do && !rc; ++a)
          std::memcpy(dst + a * D, own.data() + a * Do, Do * sizeof(double));
      }
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
// factor type present and per term group that has entries, the projected matrices and their records copied back behind
// them, one wait.  The kernel reads the window's own per-edge AtA (a term group's AtA) while that still is the linearisation
// the cache was pulled from (dense_serial, term_serial); after another linearize the cached copy is uploaded instead.  A term
// group is projected as it lies, at the group's D: a kind that owns fewer columns sits in exact zeros, which the sweeps skip
// and the acceptance test passes, and its blocks are cut from its own columns.  A factor whose record is not clean (sweep
// cap, non-finite input) is projected again on the host, so such inputs come out as sage_window_prepare_factors leaves them.
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
  // a batch per slot: the dense factor types, then the term groups
  constexpr int kSlots = 2 + plan::kTermGroups;
  struct Batch
  {
    size_t D = 0, n = 0;
    const std::vector<float> *A = nullptr; // the cached input
    std::vector<double> *C = nullptr;
    const float *dev = nullptr;            // the device's own copy, or null: it has moved on
    std::vector<SagePsdStats> rec;
  } batch[kSlots];
  const bool fresh = fc.dense_serial == w->dense_serial;
  for (int type = kPhoto; type <= kGeo; ++type)
  {
    Batch &bt = batch[type];
    bt.D = dense_dim(type, CS);
    bt.A = &fc.side[type].A;
    bt.C = &fc.side[type].C;
    bt.dev = fresh ? w->dense[type].AtA.as<float>() : nullptr;
  }
  const bool with_terms = w->terms.n_stats() > 0, fresh_terms = fc.term_serial == w->terms.serial;
  for (int g = 0; g < plan::kTermGroups; ++g)
  {
    Batch &bt = batch[2 + g];
    bt.D = (size_t)TermResults::dim(g, CS);
    bt.A = &fc.term[g].A;
    bt.C = &fc.term[g].C;
    bt.dev = with_terms && fresh_terms ? w->terms.AtA[g].as<float>() : nullptr;
  }
  int rc;
  for (int sl = 0; sl < kSlots; ++sl)
  {
    Batch &bt = batch[sl];
    bt.n = bt.A->size() / (bt.D * bt.D);
    bt.C->resize(bt.n * bt.D * bt.D);
    bt.rec.resize(bt.n);
    if (!bt.n)
      continue;
    const size_t elems = bt.n * bt.D * bt.D;
    const float *in = bt.dev;
    if (!in)
    {
      if ((rc = w->psd_in[sl].reserve(elems * sizeof(float))))
        return rc;
      SAGE_HIP(hipMemcpyAsync(w->psd_in[sl].p, bt.A->data(), elems * sizeof(float), hipMemcpyHostToDevice, w->stream));
      in = w->psd_in[sl].as<float>();
    }
    if ((rc = w->psd_out[sl].reserve(elems * sizeof(double))) || (rc = w->psd_stats[sl].reserve(bt.n * sizeof(SagePsdStats))))
      return rc;
    if ((rc = psd_project_enqueue(w->stream, (int)bt.D, (int)bt.n, in, w->psd_out[sl].as<double>(),
                                  w->psd_stats[sl].as<SagePsdStats>())))
      return rc;
    ++w->psd_launches;
  }
  for (int sl = 0; sl < kSlots; ++sl)
    if (batch[sl].n)
    {
      Batch &bt = batch[sl];
      SAGE_HIP(hipMemcpyAsync(bt.C->data(), w->psd_out[sl].p, bt.C->size() * sizeof(double), hipMemcpyDeviceToHost, w->stream));
      SAGE_HIP(hipMemcpyAsync(bt.rec.data(), w->psd_stats[sl].p, bt.n * sizeof(SagePsdStats), hipMemcpyDeviceToHost, w->stream));
    }
  SAGE_HIP(hipStreamSynchronize(w->stream));
  SagePsdStats worst_rec{};
  bool any = false;
  // the worst record: the highest status, then the most sweeps, then the most bump rounds
  auto look = [&](const SagePsdStats &r) {
    if (!any || r.status > worst_rec.status || (r.status == worst_rec.status && (r.sweeps > worst_rec.sweeps ||
        (r.sweeps == worst_rec.sweeps && r.bump_rounds > worst_rec.bump_rounds))))
      worst_rec = r;
    any = true;
  };
  for (int type = kPhoto; type <= kGeo; ++type)
    for (size_t i = 0; i < batch[type].n; ++i)
    {
      const size_t DD = batch[type].D * batch[type].D;
      look(batch[type].rec[i]);
      if (batch[type].rec[i].status != 0 && (rc = sage_factor_psd(type, CS, fc.side[type].A.data() + i * DD, 1, fc.side[type].C.data() + i * DD)))
        return rc;
    }
  if (with_terms)
  {
    std::vector<double> own;
    for (const TermRef &r : local_terms(w))
    {
      const Batch &bt = batch[2 + r.slot.group];
      if ((size_t)r.slot.out >= bt.n)
        return SAGE_E_STATE;
      look(bt.rec[r.slot.out]);
      if (bt.rec[r.slot.out].status == 0)
        continue;
      // the host's projection of the term's own matrix, into its columns of the entry
      const size_t D = bt.D, Do = (size_t)r.shape.D_own;
      own.resize(Do * Do);
      if ((rc = term_factor_psd(r.family, r.kind, CS, bt.A->data() + (size_t)r.slot.out * D * D, 1, own.data())))
        return rc;
      double *dst = term_own(bt.C->data(), r);
      for (size_t a = 0; a < Do; ++a)
        std::memcpy(dst + a * D, own.data() + a * Do, Do * sizeof(double));
    }
  }
  w->psd_worst = worst_rec;
  if (worst)
    *worst = worst_rec;
  fc.psd_mode = 1;
  return SAGE_OK;
}

extern "C" int sage_window_prepare_factors_device_launches(const SageWindow *w) { return w ? w->psd_launches : 0; }
