// window_terms.hip -- the keypoint and pose-graph terms of a window (TermSide, window_state.h): the add / num / get entry points
// of both families, stage 7 of sage_window_finalize (this rank's terms laid out by plan::term_layout, on the device behind one
// table per family) and their two launches per linearize / error pass.  Host code only.
#include "runtime_internal.h"

// ---- matched-keypoint terms ------------------------------------------------------------------------------------------
// add: arguments first (no device is touched for a bad call), then the caller's device arrays are copied to the host -- the
// locations are validated there (the kernel indexes bias / basis rows with them unchecked) -- and finalize lays this rank's
// terms out in one device pool behind one table: what lets a single launch serve them all
extern "C" int sage_window_add_keypoint_term(SageWindow *w, const SageKeypointTerm *t)
{
  if (!w || !t)
    return SAGE_E_INVALID;
  if (w->finalized)
    return SAGE_E_STATE;
  const bool rep = t->kind == SAGE_KP_REPROJECTION, mg = t->kind == SAGE_KP_MATCH_GEOMETRY, lmg = t->kind == SAGE_KP_LOOP_MG;
  if ((!rep && !mg && !lmg) || t->edge < 0 || t->edge >= 2 * (int)w->links.size() || t->N < 1 || t->N > (1 << 20) ||
      (!lmg && !t->loc1d_0) || !t->homo0 || !(t->weight >= 0.f))
    return SAGE_E_INVALID;
  if (rep && (!t->matched_2d || !(t->loss_param > 0.f)))
    return SAGE_E_INVALID;
  if (mg && (!t->matched_loc1d_1 || !t->matched_homo1 || t->loss < SAGE_LOSS_FAIR || t->loss > SAGE_LOSS_UNBIASED ||
             (t->loss != SAGE_LOSS_L2 && !(t->loss_param > 0.f))))
    return SAGE_E_INVALID;
  if (lmg && (!t->matched_homo1 || !t->unscaled_dpts0 || !t->matched_unscaled_dpts1 || !(t->loss_param > 0.f)))
    return SAGE_E_INVALID;
  KeypointTermHost h;
  h.kind = t->kind; h.edge = t->edge; h.N = t->N; h.loss = mg ? t->loss : 0;
  h.loss_param = t->loss_param; h.weight = t->weight;
  const size_t N = (size_t)t->N;
  auto fetch = [](auto &dst, const void *src, size_t n) { // a device array of the kind, or none
    dst.resize(src ? n : 0);
    return src ? hipMemcpy(dst.data(), src, n * sizeof(dst[0]), hipMemcpyDeviceToHost) : hipSuccess;
  };
  SAGE_HIP(hipStreamSynchronize(w->stream)); // (the caller may have filled the arrays on the window's stream)
  SAGE_HIP(fetch(h.loc0, lmg ? nullptr : t->loc1d_0, N));
  SAGE_HIP(fetch(h.homo0, t->homo0, 3 * N));
  SAGE_HIP(fetch(h.second, rep ? t->matched_2d : t->matched_homo1, (rep ? 2 : 3) * N));
  SAGE_HIP(fetch(h.loc1, mg ? t->matched_loc1d_1 : nullptr, N));
  SAGE_HIP(fetch(h.dpts0, lmg ? t->unscaled_dpts0 : nullptr, N));
  SAGE_HIP(fetch(h.dpts1, lmg ? t->matched_unscaled_dpts1 : nullptr, N));
  const int32_t HW = (int32_t)w->cfg.pyr.cam[0].h * (int32_t)w->cfg.pyr.cam[0].w;
  for (const std::vector<int32_t> *loc : {&h.loc0, &h.loc1})
    for (int32_t v : *loc)
      if (v < 0 || v >= HW)
        return SAGE_E_INVALID;
  w->terms.kp_added.push_back(std::move(h));
  return (int)w->terms.kp_added.size() - 1;
}

// ---- pose-graph terms ------------------------------------------------------------------------------------------------
// add: host data only -- validated and copied, no device call; finalize lays this rank's terms out in one device table
extern "C" int sage_window_add_graph_term(SageWindow *w, const SageGraphTerm *t)
{
  if (!w || !t)
    return SAGE_E_INVALID;
  if (w->finalized)
    return SAGE_E_STATE;
  const bool rps = t->kind == SAGE_GRAPH_REL_POSE_SCALE, rp = t->kind == SAGE_GRAPH_REL_POSE, sp = t->kind == SAGE_GRAPH_SCALE_PRIOR;
  if ((!rps && !rp && !sp) || !(t->weight > 0.f) || !std::isfinite(t->weight))
    return SAGE_E_INVALID;
  auto positive = [](float v) { return v > 0.f && std::isfinite(v); };
  if (sp)
  {
    if (t->kf < 0 || t->kf >= w->K || !positive(t->target_scale0))
      return SAGE_E_INVALID;
  }
  else
  {
    if (t->edge < 0 || t->edge >= 2 * (int)w->links.size() || !(t->rot_weight >= 0.f) || !std::isfinite(t->rot_weight))
      return SAGE_E_INVALID;
    for (float v : t->target_pose10)
      if (!std::isfinite(v))
        return SAGE_E_INVALID;
    if (rps && (!positive(t->target_scale0) || !positive(t->target_scale1) || !(t->scale_weight >= 0.f) ||
                !std::isfinite(t->scale_weight)))
      return SAGE_E_INVALID;
  }
  w->terms.gt_added.push_back(*t);
  return (int)w->terms.gt_added.size() - 1;
}

extern "C" int sage_window_num_keypoint_terms(const SageWindow *w) { return w ? (int)w->terms.kp_added.size() : 0; }
extern "C" int sage_window_num_graph_terms(const SageWindow *w) { return w ? (int)w->terms.gt_added.size() : 0; }

// ---- get: host copy of the last linearize of term `term` of a family: its system and {error, inliers} ----
static int term_copy_out(const SageWindow *w, bool graph, int term, float *AtA, float *Atb, float *err, float *n_in)
{
  if (!w || term < 0 || term >= (graph ? (int)w->terms.gt_added.size() : (int)w->terms.kp_added.size()))
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  const TermSide &ts = w->terms;
  const plan::TermSlot &slot = (graph ? ts.layout.graph : ts.layout.kp)[term];
  if (slot.local < 0)
    return SAGE_E_INVALID; // another rank's
  if (!ts.linearized)
    return SAGE_E_STATE;
  const TermResults res = ts.results(true);
  const size_t D = (size_t)TermResults::dim(slot.group, w->cfg.CS), out = (size_t)slot.out;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  if (AtA)
    SAGE_HIP(hipMemcpy(AtA, res.AtA(slot.group) + out * D * D, D * D * sizeof(float), hipMemcpyDeviceToHost));
  if (Atb)
    SAGE_HIP(hipMemcpy(Atb, res.Atb(slot.group) + out * D, D * sizeof(float), hipMemcpyDeviceToHost));
  float s2[2];
  SAGE_HIP(hipMemcpy(s2, res.stats + (size_t)slot.stat * 2, 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (err)
    *err = s2[0];
  if (n_in)
    *n_in = s2[1];
  return SAGE_OK;
}

extern "C" int sage_window_get_keypoint_term(const SageWindow *w, int term, float *AtA, float *Atb, float *err, float *n_in)
{
  return term_copy_out(w, false, term, AtA, Atb, err, n_in);
}

extern "C" int sage_window_get_graph_term(const SageWindow *w, int term, float *AtA, float *Atb, float *err)
{
  return term_copy_out(w, true, term, AtA, Atb, err, nullptr);
}

// ---- stage 7 of sage_window_finalize -----------------------------------------------------------------------------------
typedef std::vector<std::vector<AdjEntry>> LinkLists; // per link: the local terms on its two directions
// a term on directed edge 2 * link + direction: what the assembly walks for it -- an adjacency entry of either keyframe, an
// entry of the link's list -> its keyframes "0" (the direction's source) and "1"
static std::pair<int, int> book_on_edge(const SageWindow *w, FinalizeState &fs, LinkLists &per_link, int edge, const plan::TermSlot &slot)
{
  const int l = edge / 2, dir = edge % 2, type = plan::term_adj_type(slot.group);
  const int k0 = dir == 0 ? w->links[l].first : w->links[l].second, k1 = dir == 0 ? w->links[l].second : w->links[l].first;
  fs.adjv[k0].push_back(AdjEntry{type, slot.out, 0});
  fs.adjv[k1].push_back(AdjEntry{type, slot.out, 1});
  per_link[l].push_back(AdjEntry{type, slot.out, dir});
  fs.link_terms[l] = 1;
  return {k0, k1};
}

// pool and keypoint table: a row per local term in launch order, its arrays in the pool (4-byte words, every array 16-byte
// aligned) at the address the row holds; leaves the pool's device buffer reserved
static int keypoint_table(SageWindow *w, FinalizeState &fs, LinkLists &per_link, std::vector<uint32_t> &pool, std::vector<KpTerm> &table)
{
  TermSide &ts = w->terms;
  size_t words = 0;
  for (int id : ts.layout.kp_order)
  {
    const KeypointTermHost &h = ts.kp_added[id];
    for (size_t n : {h.loc0.size(), h.loc1.size(), h.homo0.size(), h.second.size(), h.dpts0.size(), h.dpts1.size()})
      words += (n + 3) / 4 * 4;
  }
  const int rc = ts.pool.reserve(std::max<size_t>(1, words) * sizeof(uint32_t));
  if (rc)
    return rc;
  auto put = [&pool, base = ts.pool.as<uint32_t>()](const auto &v) -> decltype(v.data()) { // an array's device address; none: null
    if (v.empty())
      return nullptr;
    const size_t off = pool.size();
    pool.resize(off + (v.size() + 3) / 4 * 4, 0u);
    std::memcpy(pool.data() + off, v.data(), v.size() * sizeof(uint32_t));
    return reinterpret_cast<decltype(v.data())>(base + off);
  };
  for (int id : ts.layout.kp_order)
  {
    const KeypointTermHost &h = ts.kp_added[id];
    const plan::TermSlot &slot = ts.layout.kp[id];
    const auto [k0, k1] = book_on_edge(w, fs, per_link, h.edge, slot);
    KpTerm kt{};
    kt.kind = h.kind; kt.loss = h.loss; kt.N = h.N;
    kt.out = slot.out; kt.stat = slot.stat;
    kt.k0 = k0; kt.k1 = k1;
    kt.loss_param = h.loss_param; kt.weight = h.weight;
    kt.loc0 = put(h.loc0); kt.loc1 = put(h.loc1); kt.homo0 = put(h.homo0);
    (h.kind == SAGE_KP_REPROJECTION ? kt.matched : kt.homo1) = put(h.second);
    kt.dpts0 = put(h.dpts0); kt.dpts1 = put(h.dpts1);
    kt.bias0 = w->views[k0].bias; kt.basis0 = w->views[k0].basis;
    kt.bias1 = w->views[k1].bias; kt.basis1 = w->views[k1].basis;
    table.push_back(kt);
    fs.residuals += (double)kp_kind_rows(h.kind) * h.N;
  }
  return SAGE_OK;
}

// graph table: a row per local term in launch order; a scale prior sits on one keyframe: an adjacency entry, no link entry
static std::vector<GraphTerm> graph_table(SageWindow *w, FinalizeState &fs, LinkLists &per_link)
{
  std::vector<GraphTerm> table;
  for (int id : w->terms.layout.graph_order)
  {
    const SageGraphTerm &h = w->terms.gt_added[id];
    const plan::TermSlot &slot = w->terms.layout.graph[id];
    GraphTerm gt{};
    gt.kind = h.kind;
    gt.out = slot.out; gt.stat = slot.stat;
    std::memcpy(gt.target, h.target_pose10, sizeof(gt.target));
    gt.ts0 = h.target_scale0; gt.ts1 = h.target_scale1;
    gt.weight = h.weight; gt.rot_weight = h.rot_weight; gt.scale_weight = h.scale_weight;
    if (h.kind == SAGE_GRAPH_SCALE_PRIOR)
    {
      gt.k0 = gt.k1 = h.kf;
      fs.adjv[h.kf].push_back(AdjEntry{plan::term_adj_type(slot.group), slot.out, 0});
    }
    else
      std::tie(gt.k0, gt.k1) = book_on_edge(w, fs, per_link, h.edge, slot);
    table.push_back(gt);
    fs.residuals += (double)graph_kind_rows(h.kind);
  }
  return table;
}

// 7. leaves this rank's terms: their layout, the pool and the two tables, the per-link lists (keypoint terms first, each family
//    in launch order), the result buffers and the zeroed {error, inliers} array; fs.adjv and fs.residuals with the terms'
//    share, fs.link_terms
int finalize_terms(SageWindow *w, FinalizeState &fs)
{
  TermSide &ts = w->terms;
  std::vector<plan::TermKey> kp, gt; // layout: a binary term is the rank's that owns its directed edge, a scale prior rank 0's
  for (const KeypointTermHost &h : ts.kp_added)
    kp.push_back({h.kind, window_owns_edge(w, h.edge)});
  for (const SageGraphTerm &h : ts.gt_added)
    gt.push_back({h.kind, h.kind == SAGE_GRAPH_SCALE_PRIOR ? w->rank == 0 : window_owns_edge(w, h.edge)});
  ts.layout = plan::term_layout(kp, gt);
  fs.link_terms.assign(w->links.size(), 0);
  if (ts.n_stats() == 0)
    return SAGE_OK;
  LinkLists per_link(w->links.size());
  std::vector<uint32_t> pool;
  std::vector<KpTerm> kp_table;
  int rc;
  if ((rc = keypoint_table(w, fs, per_link, pool, kp_table)))
    return rc;
  const std::vector<GraphTerm> gt_table = graph_table(w, fs, per_link);
  std::vector<int32_t> link_start{0};
  std::vector<AdjEntry> link;
  for (const std::vector<AdjEntry> &l : per_link)
  {
    link.insert(link.end(), l.begin(), l.end());
    link_start.push_back((int32_t)link.size());
  }
  if ((rc = upload(ts.pool, pool, w->stream)) || (rc = upload(ts.kp_table, kp_table, w->stream)) ||
      (rc = upload(ts.gt_table, gt_table, w->stream)) || (rc = upload(ts.link_start, link_start, w->stream)) ||
      (rc = upload(ts.link, link, w->stream)) || (rc = ts.reserve_results(w->cfg.CS, w->stream)))
    return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream)); // (the host vectors go out of scope)
  return SAGE_OK;
}

// ---- the two batched kernels over this rank's terms at variable set `set`: keypoint terms, then graph terms; jac: the
//      linearize (profiler slots 4 / 6), else the error pass (5 / 7)
template <class Launch>
static int timed_launch(SageWindow *w, int slot, Launch launch)
{
  LaunchCommon lc{};
  prof_attach(w, slot, lc);
  if (lc.ev_start)
    (void)hipEventRecord(lc.ev_start, w->stream);
  SAGE_HIP(launch());
  if (lc.ev_stop)
    (void)hipEventRecord(lc.ev_stop, w->stream);
  return SAGE_OK;
}

int window_launch_terms(SageWindow *w, int set, bool jac)
{
  TermSide &ts = w->terms;
  const float *vars = w->vars[set].as<float>();
  const KpBatchParams kp{ts.kp_table.as<KpTerm>(), vars, w->VS, w->cfg.pyr.cam[0], w->cfg.eps, ts.results(jac)};
  const GraphBatchParams gp{ts.gt_table.as<GraphTerm>(), ts.n_graph(), vars, w->VS, ts.results(jac)};
  int rc = SAGE_OK;
  if (jac && ts.n_stats() > 0)
    ++ts.serial; // the groups' AtA are about to be rewritten
  if (ts.n_keypoint() > 0)
    rc = timed_launch(w, jac ? 4 : 5, [&] {
      return launch_keypoint_batch(w->stream, w->cfg.CS, jac, ts.n_keypoint(), ts.keypoint_kinds(), kp);
    });
  if (ts.n_graph() > 0 && !rc)
    rc = timed_launch(w, jac ? 6 : 7, [&] { return launch_graph_terms(w->stream, jac, gp); });
  ts.linearized |= jac && ts.n_stats() > 0 && !rc;
  return rc;
}
