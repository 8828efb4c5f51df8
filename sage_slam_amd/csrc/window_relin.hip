// window_relin.hip -- partial relinearization of a finalized window (SAGE_RELIN_STALE), as ISAM2 relinearizes: which dense edges
// a linearize has to evaluate (the reads table of relin_plan.h against the snapshot of the values the per-edge results stand
// for), the depth maps those edges read (rebuilt by stamp), the compacted launch plan and the kernel that writes it, and the
// host side of ISAM2's fluid loop: the relinearization marks of the last solve's delta and the masked accept.
// window_linearize_set (window_eval.hip) launches what relin_prepare leaves; the main kernels and the assembly are unchanged.
#include "damped_system.h"
#include "relin_plan.h"
#include "runtime_internal.h"

namespace sage
{

// One workgroup per stale edge: its work items move from the full list to the sub list, in the stale edges' order, and the
// edge's entry of the full-length first_sub (rec_first_sub: of the photometric record plan) gets its compacted offset.  The
// entries of clean edges are not touched -- and not read: the finalize handles the listed edges only.
struct RelinCompactParams
{
  const WorkItem *work;                    // the full list (DenseSide::work, first, tiles)
  const int32_t *first, *tiles;
  const int32_t *list, *item_off, *rec_off; // [n_active]: the stale edges, their first sub item, their first sub record (or null)
  WorkItem *work_sub;                      // [cap_items]
  int32_t *first_sub, *rec_first_sub;      // [n_edges]; rec_first_sub null without a record plan
  int n_active, n_edges, cap_items;
};

__global__ __launch_bounds__(64) void relin_compact_kernel(const RelinCompactParams p)
{
  const int j = (int)blockIdx.x;
  if (j >= p.n_active)
    return;
  const int e = p.list[j];
  if (e < 0 || e >= p.n_edges)
    return;
  const int src = p.first[e], n = p.tiles[e], dst = p.item_off[j];
  for (int i = (int)threadIdx.x; i < n; i += 64)
    if (dst + i < p.cap_items) // (the host's offsets are sums of the same `tiles`: never past the list)
      p.work_sub[dst + i] = p.work[src + i];
  if (threadIdx.x == 0)
  {
    p.first_sub[e] = dst;
    if (p.rec_first_sub)
      p.rec_first_sub[e] = p.rec_off[j];
  }
}

} // namespace sage

static void relin_invalidate_stamps(RelinSide &r)
{
  std::fill(r.map_ok.begin(), r.map_ok.end(), 0);
  std::fill(r.grad_ok.begin(), r.grad_ok.end(), 0);
}

// host vectors and device buffers of the mode, sized for the window as it is now (the photometric work list grows and
// shrinks with sage_window_set_runs); nothing happens once they are large enough
static int relin_reserve(SageWindow *w)
{
  RelinSide &r = w->relin;
  const size_t K = (size_t)w->K, CS = (size_t)w->cfg.CS, ne = std::max(1, w->n_edges);
  if (r.map_ok.size() != K)
  {
    r.pose.assign(K * 12, 0.f); r.code.assign(K * CS, 0.f); r.scale.assign(K, 0.f);
    r.map_code.assign(K * CS, 0.f); r.map_scale.assign(K, 0.f);
    r.map_ok.assign(K, 0); r.grad_ok.assign(K, 0);
    r.drop();
    const size_t HW = (size_t)w->cfg.pyr.cam[0].h * (size_t)w->cfg.pyr.cam[0].w;
    r.depth_items.clear();
    for (size_t k = 0; k < K; ++k) // (what finalize puts into depth_items[0], for every keyframe)
    {
      const float *vp = w->vars[0].as<float>() + k * w->VS;
      r.depth_items.push_back(DepthItem{w->views[k].bias, w->views[k].basis, vp + 13, vp + 12, w->dpt.as<float>() + k * HW,
                                        w->dgrad.as<float>() + k * 2 * HW});
    }
  }
  int rc;
  for (int t = 0; t < 2; ++t)
  {
    const bool fresh = r.first_sub[t].cap < ne * sizeof(int32_t);
    if ((rc = r.work_sub[t].reserve(std::max(1, w->dense[t].n_work) * sizeof(WorkItem))) ||
        (rc = r.first_sub[t].reserve(ne * sizeof(int32_t))))
      return rc;
    if (fresh)
      SAGE_HIP(hipMemsetAsync(r.first_sub[t].p, 0, ne * sizeof(int32_t), w->stream));
  }
  const bool fresh = r.rec_first_sub.cap < ne * sizeof(int32_t);
  if ((rc = r.rec_first_sub.reserve(ne * sizeof(int32_t))) || (rc = r.lists.reserve(5 * ne * sizeof(int32_t))) ||
      (rc = r.stage_lists.reserve(5 * ne * sizeof(int32_t))) || (rc = r.depth_sub.reserve(2 * K * sizeof(DepthItem))) ||
      (rc = r.stage_depth.reserve(2 * K * sizeof(DepthItem))))
    return rc;
  if (fresh)
    SAGE_HIP(hipMemsetAsync(r.rec_first_sub.p, 0, ne * sizeof(int32_t), w->stream));
  if (!r.stage_free)
    SAGE_HIP(hipEventCreateWithFlags(&r.stage_free, hipEventDisableTiming));
  return SAGE_OK;
}

extern "C" int sage_window_set_relinearization(SageWindow *w, int mode)
{
  if (!w || (mode != SAGE_RELIN_ALL && mode != SAGE_RELIN_STALE))
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  if (mode == SAGE_RELIN_STALE && w->world > 1)
    return SAGE_E_UNSUPPORTED;
  RelinSide &r = w->relin;
  if (mode == r.mode)
    return SAGE_OK;
  r.mode = mode;
  r.drop(); // a switch: every edge is stale, no depth map is known
  relin_invalidate_stamps(r);
  return mode == SAGE_RELIN_STALE ? relin_reserve(w) : SAGE_OK;
}

extern "C" int sage_window_last_evaluation(const SageWindow *w, SageEvalCounts *out)
{
  if (!w || !out)
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  *out = w->relin.counts;
  return SAGE_OK;
}

void relin_count_all(SageWindow *w, bool dense, bool depth, bool grad)
{
  SageEvalCounts &n = w->relin.counts;
  n = SageEvalCounts{};
  if (!dense)
    return;
  const SageWindowConfig &c = w->cfg;
  n.photo_edges = c.use_photo ? w->n_edges : 0;
  n.geo_edges = c.use_geo ? w->n_edges : 0;
  n.photo_items = c.use_photo ? w->dense[kPhoto].n_work : 0;
  n.geo_items = c.use_geo ? w->dense[kGeo].n_work : 0;
  n.depth_maps = depth ? w->n_depth : 0;
  n.depth_grads = grad ? w->n_depth : 0;
}

// a whole-window depth batch at variable set `set` has been enqueued (linearize of every edge, error pass, the speculated
// gradients): every map's stamp is that set's code and scale -- unless the set is a candidate whose host mirror is still on
// its way (the device solver's), then no map is known
void relin_stamp_maps(SageWindow *w, int set, bool depth, bool grad)
{
  RelinSide &r = w->relin;
  if (r.mode != SAGE_RELIN_STALE || r.map_ok.empty())
    return;
  const bool known = !(set == 1 && w->cand_pending);
  if (depth)
  {
    if (known)
    {
      r.map_code = w->hv.code[set];
      r.map_scale = w->hv.scale[set];
    }
    std::fill(r.map_ok.begin(), r.map_ok.end(), known ? 1 : 0);
    std::fill(r.grad_ok.begin(), r.grad_ok.end(), known && grad ? 1 : 0);
  }
  else if (grad)
    r.grad_ok = r.map_ok;
}

int relin_prepare(SageWindow *w, RelinLaunch &rl)
{
  RelinSide &r = w->relin;
  const SageWindowConfig &c = w->cfg;
  const int K = w->K, CS = c.CS, ne = w->n_edges;
  int rc;
  if ((rc = relin_reserve(w)))
    return rc;
  r.counts = SageEvalCounts{};
  r.evaluated[kPhoto].clear();
  r.evaluated[kGeo].clear();
  // 1. the groups that differ from the snapshot
  std::vector<uint8_t> ch((size_t)K, 7);
  if (r.valid)
    ch = plan::changed_groups(K, CS, r.pose.data(), r.code.data(), r.scale.data(), w->hv.pose[0].data(), w->hv.code[0].data(),
                              w->hv.scale[0].data());
  const bool same = std::all_of(ch.begin(), ch.end(), [](uint8_t m) { return m == 0; });
  if (same && w->have_lin && r.packed_current)
  {
    rl.nothing = true;
    return SAGE_OK;
  }
  // 2. the stale edges of each factor type, and the depth maps they read
  const std::vector<int32_t> lk = window_link_pairs(w);
  std::vector<uint8_t> need_map((size_t)K, 0), need_grad((size_t)K, 0);
  for (int le = 0; le < ne; ++le)
  {
    int src, dst;
    plan::edge_ends(lk.data(), w->local_edges[le], &src, &dst);
    const bool ps = c.use_photo && plan::photo_edge_stale(ch[src], ch[dst]);
    const bool gs = c.use_geo && plan::geo_edge_stale(ch[src], ch[dst]);
    if (ps)
      r.evaluated[kPhoto].push_back(le);
    if (gs)
      r.evaluated[kGeo].push_back(le);
    plan::edge_map_reads(src, dst, ps, gs, need_map.data(), need_grad.data());
  }
  const int np = (int)r.evaluated[kPhoto].size(), ng = (int)r.evaluated[kGeo].size();
  if (np + ng == 0)
    return SAGE_OK; // (the terms and the assembly still run: a keyframe without a dense edge may have moved)
  // the staging memory of the previous call has been copied from (an event, not a synchronise: the stream may run ahead)
  if (r.stage_busy)
    SAGE_HIP(hipEventSynchronize(r.stage_free));
  // 3. the maps to rebuild: a map a launched edge reads whose stamp is not the current code and scale; a gradient a launched
  //    geometric edge reads that was not built from the map as it is
  DepthItem *items = r.stage_depth.as<DepthItem>();
  int nd = 0, ngr = 0;
  for (int pass = 0; pass < 2; ++pass) // (the maps' items first, the gradients' behind them)
    for (int k = 0; k < K; ++k)
    {
      if (pass == 0 && need_map[k])
      {
        const float *code = &w->hv.code[0][(size_t)k * CS];
        const bool fresh = r.map_ok[k] && std::memcmp(&r.map_code[(size_t)k * CS], code, CS * sizeof(float)) == 0 &&
                           std::memcmp(&r.map_scale[k], &w->hv.scale[0][k], sizeof(float)) == 0;
        if (!fresh)
        {
          items[nd++] = r.depth_items[k];
          std::memcpy(&r.map_code[(size_t)k * CS], code, CS * sizeof(float));
          r.map_scale[k] = w->hv.scale[0][k];
          r.map_ok[k] = 1;
          r.grad_ok[k] = 0;
        }
      }
      if (pass == 1 && need_grad[k] && !r.grad_ok[k])
      {
        items[nd + ngr++] = r.depth_items[k];
        r.grad_ok[k] = 1;
      }
    }
  // 4. per side: the stale edges and the exclusive offsets of their work items (photometric: and of their records)
  int32_t *st = r.stage_lists.as<int32_t>();
  const bool records = c.use_photo && w->photo_rec.flush > 0;
  size_t at = 0;
  size_t list_at[2] = {0, 0}, off_at[2] = {0, 0}, rec_at = 0;
  for (int t = 0; t < 2; ++t)
  {
    const std::vector<int32_t> &ev = r.evaluated[t], &tiles = w->dense[t].h_tiles;
    list_at[t] = at;
    std::copy(ev.begin(), ev.end(), st + at);
    at += ev.size();
    off_at[t] = at;
    int items_t = 0;
    for (int32_t e : ev)
    {
      st[at++] = items_t;
      items_t += tiles[e];
    }
    rl.n_edges[t] = (int)ev.size();
    rl.n_items[t] = items_t;
    if (t == kPhoto && records)
    {
      rec_at = at;
      int recs = 0;
      for (int32_t e : ev)
      {
        st[at++] = recs;
        recs += w->photo_rec.h_count[e];
      }
    }
  }
  if (at)
    SAGE_HIP(hipMemcpyAsync(r.lists.p, st, at * sizeof(int32_t), hipMemcpyHostToDevice, w->stream));
  if (nd + ngr)
    SAGE_HIP(hipMemcpyAsync(r.depth_sub.p, items, (size_t)(nd + ngr) * sizeof(DepthItem), hipMemcpyHostToDevice, w->stream));
  SAGE_HIP(hipEventRecord(r.stage_free, w->stream));
  r.stage_busy = true;
  const int32_t *lists = r.lists.as<int32_t>();
  for (int t = 0; t < 2; ++t)
  {
    if (!rl.n_edges[t])
      continue;
    const DenseSide &sd = w->dense[t];
    const bool rec = t == kPhoto && records;
    RelinCompactParams p{};
    p.work = sd.work.as<WorkItem>(); p.first = sd.first.as<int32_t>(); p.tiles = sd.tiles.as<int32_t>();
    p.list = lists + list_at[t]; p.item_off = lists + off_at[t]; p.rec_off = rec ? lists + rec_at : nullptr;
    p.work_sub = r.work_sub[t].as<WorkItem>();
    p.first_sub = r.first_sub[t].as<int32_t>();
    p.rec_first_sub = rec ? r.rec_first_sub.as<int32_t>() : nullptr;
    p.n_active = rl.n_edges[t]; p.n_edges = ne; p.cap_items = sd.n_work;
    hipLaunchKernelGGL(relin_compact_kernel, dim3(p.n_active), dim3(64), 0, w->stream, p);
    SAGE_HIP(hipGetLastError());
    rl.work[t] = p.work_sub;
    rl.first[t] = rec ? p.rec_first_sub : p.first_sub;
    rl.list[t] = p.list;
  }
  // 5. the depth batch of the keyframes whose stamp does not match, then the gradients (they read the maps just written)
  const int H = (int)c.pyr.cam[0].h, W = (int)c.pyr.cam[0].w;
  SAGE_HIP(launch_depth_batch(w->stream, CS, r.depth_sub.as<DepthItem>(), nd, H, W, true, false));
  SAGE_HIP(launch_depth_batch(w->stream, CS, r.depth_sub.as<DepthItem>() + nd, ngr, H, W, false, true));
  if (nd)
  {
    // the maps are a mix now: the current set's where rebuilt, whatever they held elsewhere
    w->dpt_set = w->dpt_set == 0 ? 0 : -1;
    w->dgrad_valid = false;
  }
  SageEvalCounts &n = r.counts;
  n.photo_edges = rl.n_edges[kPhoto]; n.geo_edges = rl.n_edges[kGeo];
  n.photo_items = rl.n_items[kPhoto]; n.geo_items = rl.n_items[kGeo];
  n.depth_maps = nd; n.depth_grads = ngr;
  return SAGE_OK;
}

void relin_commit(SageWindow *w, const RelinLaunch &)
{
  RelinSide &r = w->relin;
  r.pose = w->hv.pose[0];
  r.code = w->hv.code[0];
  r.scale = w->hv.scale[0];
  r.valid = r.packed_current = true;
}

// ---- ISAM2's fluid loop on the host: which groups the last solve's delta moves past their thresholds, and the accept of
//      those groups alone
extern "C" int sage_window_relin_marks(const SageWindow *w, const SageRelinThresholds *t, int32_t *marks, int32_t *n_marked)
{
  if (!w || !t || !marks)
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  if (const int rcs = window_sync_candidate(const_cast<SageWindow *>(w)))
    return rcs;
  int32_t n = 0;
  for (int k = 0; k < w->K; ++k)
  {
    const int hold = w->hold.empty() ? 0 : w->hold[k]; // (gtsam erases fixedVariables from the set)
    const int m = plan::relin_marks_of(&w->delta[(size_t)k * w->B], w->cfg.CS, t->pose, t->code, t->scale) & ~hold;
    marks[k] = m;
    n += (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1);
  }
  if (n_marked)
    *n_marked = n;
  return SAGE_OK;
}

extern "C" int sage_window_accept_marked(SageWindow *w, const int32_t *marks)
{
  if (!w || !marks)
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  const int K = w->K, CS = w->cfg.CS;
  for (int k = 0; k < K; ++k)
    if (marks[k] < 0 || marks[k] > (SAGE_HOLD_POSE | SAGE_HOLD_CODE | SAGE_HOLD_SCALE))
      return SAGE_E_INVALID;
  int rc = window_sync_candidate(w);
  if (rc)
    return rc;
  HostVars &hv = w->hv;
  for (int k = 0; k < K; ++k)
  {
    const int m = marks[k] & ~(w->hold.empty() ? 0 : (int)w->hold[k]);
    if (m & sage::kHoldPose)
      std::copy_n(&hv.pose[1][(size_t)k * 12], 12, &hv.pose[0][(size_t)k * 12]);
    if (m & sage::kHoldCode)
      std::copy_n(&hv.code[1][(size_t)k * CS], CS, &hv.code[0][(size_t)k * CS]);
    if (m & sage::kHoldScale)
      hv.scale[0][k] = hv.scale[1][k];
  }
  hv.copy_set(1, 0); // the unmarked groups of the candidate are dropped: both sets are the new linearization point
  w->dogleg.solved0 = w->dogleg.products = false; // (as sage_window_accept)
  if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
    return rc;
  return SAGE_OK;
}
