// window_build.hip -- the build-time half of the window engine: create / destroy, keyframes and links as they are added (terms:
// window_terms.hip), sage_window_finalize as a list of stages (its policy: window_plan.h), the photometric run plan and its tuning.  Host
// code only: kernels are reached through the launch_* wrappers; what runs on a finalized window is window_eval / _reduce / _solve / _lm.hip.
#include "runtime_internal.h"
#include "window_plan.h"

// live windows of the process: the last sage_window_destroy stops the solver's host threads (host_threads.cpp "life cycle")
static std::atomic<int> g_live_windows{0};

extern "C" int sage_window_create(const SageWindowConfig *cfg, void *hip_stream, SageWindow **out)
{
  if (!cfg || !out || !cfg->mask_dev)
    return SAGE_E_INVALID;
  if (!supported(cfg->CS, cfg->FS) || cfg->pyr.levels < 1 || cfg->pyr.levels > SAGE_MAX_LEVELS)
    return SAGE_E_UNSUPPORTED;
  int ndev = 0;
  SAGE_HIP(hipGetDeviceCount(&ndev));
  if (ndev < 1)
    return (int)hipErrorNoDevice;
  SageWindow *w = new SageWindow();
  w->cfg = *cfg;
  w->stream = reinterpret_cast<hipStream_t>(hip_stream);
  w->B = 7 + cfg->CS;
  w->VS = ((13 + cfg->CS + 3) / 4) * 4;
  *out = w;
  g_live_windows.fetch_add(1, std::memory_order_acq_rel);
  return SAGE_OK;
}

extern "C" void sage_window_destroy(SageWindow *w)
{
  if (!w)
    return;
  // no thread of this library outlives the last window (r06): helpers, arrow-row pool and the opt-in
  // placement monitor are stopped and joined; the next window's first solve starts them again
  struct LastOut
  {
    ~LastOut()
    {
      if (g_live_windows.fetch_sub(1, std::memory_order_acq_rel) == 1)
        sage::host_threads_shutdown();
    }
  } last_out;
  // device buffers, the pinned mirror and the profiler's events go with their owners (DevBuf, TotalsMirror, WindowProfiler)
  std::free(w->dist.rccl_hook); // (the communicator itself belongs to the caller)
  for (SagePreparedKeyframe *pk : w->prepared)
    prepared_release(pk); // (null: a keyframe added as a view)
  sage_shard_plan_destroy(w->dist.shard);
  solver_destroy(w->solver);
  delete w;
}

// a keyframe's arrays, its handle (null: added as a view) and its variables
static int add_keyframe(SageWindow *w, const SageKeyframeView *v, SagePreparedKeyframe *pk, const float *pose12, const float *code,
                        float scale)
{
  w->views.push_back(*v);
  w->prepared.push_back(pk);
  for (int s = 0; s < 2; ++s)
  {
    w->hv.pose[s].insert(w->hv.pose[s].end(), pose12, pose12 + 12);
    w->hv.code[s].insert(w->hv.code[s].end(), code, code + w->cfg.CS);
    w->hv.scale[s].push_back(scale);
  }
  w->hv.pose_init.insert(w->hv.pose_init.end(), pose12, pose12 + 12);
  w->hv.code_added.insert(w->hv.code_added.end(), code, code + w->cfg.CS);
  w->hv.scale_init.push_back(scale);
  return w->K++;
}

extern "C" int sage_window_add_keyframe(SageWindow *w, const SageKeyframeView *v, const float *pose12,
                                        const float *code, float scale)
{
  if (!w || !v || !pose12 || !code || w->finalized)
    return SAGE_E_INVALID;
  if (!v->feat_pyr || !v->grad_pyr || !v->bias || !v->basis || !v->loc1d || !v->homo || v->N < 0)
    return SAGE_E_INVALID;
  return add_keyframe(w, v, nullptr, pose12, code, scale);
}

// a keyframe by its handle: the window borrows the handle's planes, ordered samples and pre-sampled features instead of making
// its own (stages 3-5 of finalize skip it) and holds a reference until it is destroyed.  Only a handle prepared under the
// window's pyr / FS / photo_weights and the process's sample switches holds what the window itself would have made
extern "C" int sage_window_add_prepared_keyframe(SageWindow *w, SagePreparedKeyframe *pk, const float *pose12, const float *code,
                                                 float scale)
{
  if (!w || !pk || !pose12 || !code)
    return SAGE_E_INVALID;
  if (w->finalized)
    return SAGE_E_STATE;
  if (!prep::same_fingerprint(pk->fp, prep::fingerprint(w->cfg, prep::sample_switches())))
    return SAGE_E_INVALID;
  prepared_retain(pk);
  return add_keyframe(w, &pk->view, pk, pose12, code, scale);
}

extern "C" int sage_window_build_stats(const SageWindow *w, SageWindowBuildStats *out)
{
  if (!w || !out)
    return SAGE_E_INVALID;
  *out = w->build_stats;
  return SAGE_OK;
}

// a link: part of the solver's structure and of the packed buffer; dense = 0: keypoint terms only, no row of the dense edge tables
static int add_link(SageWindow *w, int a, int b, char dense)
{
  if (a == b || a < 0 || b < 0 || a >= w->K || b >= w->K)
    return SAGE_E_INVALID;
  w->links.emplace_back(std::min(a, b), std::max(a, b));
  w->link_geo_loss.push_back(0.f);
  w->link_dense.push_back(dense);
  return (int)w->links.size() - 1;
}

extern "C" int sage_window_add_link(SageWindow *w, int a, int b) { return !w || w->finalized ? SAGE_E_INVALID : add_link(w, a, b, 1); }
extern "C" int sage_window_add_keypoint_link(SageWindow *w, int a, int b)
{
  return !w ? SAGE_E_INVALID : (w->finalized ? SAGE_E_STATE : add_link(w, a, b, 0));
}

extern "C" int sage_window_hold(SageWindow *w, int kf, int what)
{
  if (!w)
    return SAGE_E_INVALID;
  if (w->finalized)
    return SAGE_E_STATE;
  if (kf < 0 || kf >= w->K || what < 0 || what > (SAGE_HOLD_POSE | SAGE_HOLD_CODE | SAGE_HOLD_SCALE))
    return SAGE_E_INVALID;
  w->hold.resize(w->K, 0); // (keyframes added since the last call: free)
  w->hold[kf] = (uint8_t)what;
  return SAGE_OK;
}

extern "C" int sage_window_set_link_geo_loss(SageWindow *w, int link, float loss_param)
{
  if (!w || w->finalized || link < 0 || link >= (int)w->links.size() || !(loss_param >= 0.f))
    return w && w->finalized ? SAGE_E_STATE : SAGE_E_INVALID;
  w->link_geo_loss[link] = loss_param;
  return SAGE_OK;
}

// ---- photometric run plan (work list of the photometric linearize / error pass) ------------------------------------------------
// record cadence of a run length: the plan's, unless SAGE_PHOTO_FLUSH sets one
static int photo_flush_for_runs(int tpb)
{
  if (const char *e = getenv("SAGE_PHOTO_FLUSH"))
    return std::max(0, atoi(e));
  return plan::record_cadence(tpb);
}

// a side's work list: items, per edge its first item and its number of items (the caller synchronises before `wl` dies)
static int upload_work_list(DenseSide &sd, const WorkList &wl, hipStream_t s)
{
  int rc;
  sd.n_work = (int)wl.work.size();
  sd.tpb = wl.tiles_per_block;
  sd.h_tiles = wl.edge_tiles;
  if ((rc = upload(sd.work, wl.work, s)) || (rc = upload(sd.first, wl.edge_first, s)) || (rc = upload(sd.tiles, wl.edge_tiles, s)))
    return rc;
  return SAGE_OK;
}

// what was assembled or evaluated under the previous photometric plan is not this plan's: another run length sums in another
// fp32 order, so `packed`, the error kept for the linearize-at-candidate sequence and the depth maps' booking are dropped
static void window_invalidate_plan_results(SageWindow *w)
{
  w->have_lin = false;
  w->spec_err_valid = false;
  w->dpt_set = -1;
}

// (re)build the photometric work list for runs of `tpb` sub-tiles and upload it; the partial-record buffer grows to fit
static int window_plan_photo_runs(SageWindow *w, int tpb, int flush)
{
  WorkList wp;
  wp.build(w->Nedge, tpb, nullptr, flush);
  int rc;
  w->photo_rec.flush = wp.flush;
  w->photo_rec.n = wp.n_records;
  w->photo_rec.h_count = wp.rec_count;
  w->relin.drop(); // the record layout changes: no per-edge result is this plan's
  DenseSide &ph = w->dense[kPhoto];
  if ((rc = upload_work_list(ph, wp, w->stream)) || (rc = upload(w->photo_rec.first, wp.rec_first, w->stream)) ||
      (rc = upload(w->photo_rec.count, wp.rec_count, w->stream)))
    return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream)); // (the host vectors go out of scope)
  return ph.part.reserve(std::max<size_t>(1, std::max(ph.n_work, w->photo_rec.n)) * photo_partial_floats(w->cfg.CS) * sizeof(float));
}

// edge lengths in the plan's unit: sub-tiles per edge
static std::vector<int> edge_tiles(const std::vector<int> &Nedge)
{
  std::vector<int> tiles;
  for (int n : Nedge)
    tiles.push_back((n + kTile - 1) / kTile);
  return tiles;
}

// ---- sage_window_finalize: stages in stream order.  Every stage returns SAGE_OK, a SAGE_E_* code or a hipError_t, synchronises
//      the stream before a host vector it uploaded from dies, and can run again after a finalize that failed.  What the stages
//      hand to one another is FinalizeState (runtime_internal.h); stage 7, the terms, is window_terms.hip's finalize_terms
static int image_pixels(const SageWindow *w) { return (int)w->cfg.pyr.cam[0].h * (int)w->cfg.pyr.cam[0].w; }

// 1. leaves both variable sets on the device and room for every keyframe's depth map and its gradients
static int finalize_variables(SageWindow *w)
{
  const int K = w->K, HW = image_pixels(w);
  int rc;
  for (int s = 0; s < 2; ++s)
  {
    if ((rc = w->vars[s].reserve((size_t)K * w->VS * sizeof(float))))
      return rc;
    if ((rc = window_upload_vars(w, s)))
      return rc;
  }
  if ((rc = w->dpt.reserve((size_t)K * HW * sizeof(float))) || (rc = w->dgrad.reserve((size_t)K * 2 * HW * sizeof(float))))
    return rc;
  return SAGE_OK;
}

// 2. leaves owned_edges / local_links (plan::owned_edges), local_edges (plan::dense_edges), fs.needed (the keyframes this
//    rank's DENSE edges touch), n_depth and the depth items of both variable sets.
//    Whole links on request (SAGE_SHARD_BY_LINK) and for windows whose domain-decomposed solve derives its domains from them
static int finalize_ownership(SageWindow *w, FinalizeState &fs)
{
  const int K = w->K, HW = image_pixels(w);
  int rc;
  const bool by_link = sage::env_flag("SAGE_SHARD_BY_LINK") || fs.domain_solve;
  plan::Ownership own = plan::owned_edges((int)w->links.size(), w->rank, w->world, by_link);
  w->owned_edges = std::move(own.edges);
  w->local_links = std::move(own.links);
  w->local_edges = plan::dense_edges(w->owned_edges, w->link_dense);
  fs.needed.assign(K, 0);
  for (int ge : w->local_edges)
    fs.needed[w->links[ge / 2].first] = fs.needed[w->links[ge / 2].second] = 1;
  w->n_depth = 0;
  for (int k = 0; k < K; ++k)
    w->n_depth += fs.needed[k];
  for (int s = 0; s < 2; ++s)
  {
    std::vector<DepthItem> items;
    for (int k = 0; k < K; ++k)
    {
      if (!fs.needed[k])
        continue;
      const float *vp = w->vars[s].as<float>() + (size_t)k * w->VS;
      items.push_back(DepthItem{w->views[k].bias, w->views[k].basis, vp + 13, vp + 12,
                                w->dpt.as<float>() + (size_t)k * HW, w->dgrad.as<float>() + (size_t)k * 2 * HW});
    }
    if ((rc = upload(w->depth_items[s], items, w->stream)))
      return rc;
    SAGE_HIP(hipStreamSynchronize(w->stream));
  }
  return SAGE_OK;
}

// 3. leaves pk: the engine-internal relayout, once per keyframe: [FS][P] -> [FS/4][P][4] for feat, grad-x, grad-y (and rejects a
//    negative photometric level weight)
static int finalize_pyramids(SageWindow *w)
{
  const SageWindowConfig &c = w->cfg;
  const int FS = c.FS, K = w->K;
  int rc;
  const size_t plane_f = (size_t)FS * c.pyr.P;
  const size_t n_views = std::count(w->prepared.begin(), w->prepared.end(), nullptr); // (a prepared keyframe brings its planes)
  if ((rc = w->pk.reserve(n_views * 3 * plane_f * sizeof(float))))
    return rc;
  // r05: every texel of level l also carries sqrt(w_l) (feat, fx d/dx, fy d/dy -- and with feat the pre-sampled source
  // features of stage 5): the products the kernels sum (h h^T, h r, r^2) then hold the level weight of
  // photometric_factor_kernels.cpp:1143-1149 by themselves -- no per-step weighting in the kernels' sampling loops
  float lvl_scale[SAGE_MAX_LEVELS] = {};
  for (int l = 0; l < c.pyr.levels; ++l)
  {
    if (!(c.photo_weights[l] >= 0.f))
      return SAGE_E_INVALID;
    lvl_scale[l] = std::sqrt(c.photo_weights[l]);
  }
  w->kf_pk.assign(K, nullptr);
  size_t vi = 0; // views before keyframe k
  for (int k = 0; k < K; ++k)
  {
    if (w->prepared[k])
    {
      w->kf_pk[k] = w->prepared[k]->pk;
      continue;
    }
    float *base = w->pk.as<float>() + vi++ * 3 * plane_f;
    SAGE_HIP(launch_repack_groups(w->stream, base, w->views[k].feat_pyr, FS, c.pyr.P, 0, &c.pyr, lvl_scale));
    SAGE_HIP(launch_repack_groups(w->stream, base + plane_f, w->views[k].grad_pyr, FS, c.pyr.P, 1, &c.pyr, lvl_scale));
    SAGE_HIP(launch_repack_groups(w->stream, base + 2 * plane_f, w->views[k].grad_pyr + plane_f, FS, c.pyr.P, 2, &c.pyr, lvl_scale));
    w->kf_pk[k] = base;
    w->build_stats.repacked += 1;
    w->build_stats.launches += 3;
  }
  return SAGE_OK;
}

// 4. leaves sorted_loc / sorted_homo and the views pointing at them: the sampled locations validated (the kernels index depth
//    maps / basis rows with them unchecked) and relaid in tile order (engine-owned copies; see producers.hip: the sums are order
//    independent, the L1 is not); views[k].N becomes the slot count of a keyframe relaid with holes
static int finalize_samples(SageWindow *w)
{
  const SageWindowConfig &c = w->cfg;
  const int K = w->K, HW = image_pixels(w);
  int rc;
  if ((int)w->user_samples.size() != K) // (a retried finalize must not sort the sorted copies onto themselves)
  {
    w->user_samples.resize(K);
    w->user_n.resize(K);
    for (int k = 0; k < K; ++k)
    {
      w->user_samples[k] = {w->views[k].loc1d, w->views[k].homo};
      w->user_n[k] = w->views[k].N;
    }
  }
  for (int k = 0; k < K; ++k)
    w->views[k].N = w->user_n[k];
  // a prepared keyframe brings its ordered samples (validated when it was prepared): the relay below is the views' alone
  std::vector<int> vk; // the keyframes added as views, ascending
  for (int k = 0; k < K; ++k)
  {
    const SagePreparedKeyframe *h = w->prepared[k];
    if (!h)
    {
      vk.push_back(k);
      continue;
    }
    w->views[k].N = h->slots;
    w->views[k].loc1d = h->loc;
    w->views[k].homo = h->homo;
  }
  const int Kv = (int)vk.size();
  if (Kv == 0)
    return SAGE_OK;
  // (capacity per keyframe: its samples, or -- tile-padded order -- every 8 x 8 tile of the image with all 64 slots)
  const size_t cap_tiles = (size_t)(((int)c.pyr.cam[0].w + 7) / 8) * (size_t)(((int)c.pyr.cam[0].h + 7) / 8) * 64;
  std::vector<size_t> soff(Kv + 1, 0);
  int max_n = 0;
  for (int j = 0; j < Kv; ++j)
  {
    soff[j + 1] = soff[j] + std::max<size_t>(std::max(1, w->views[vk[j]].N), cap_tiles);
    max_n = std::max(max_n, w->views[vk[j]].N);
  }
  if ((rc = w->sorted_loc.reserve(soff[Kv] * sizeof(int64_t))) || (rc = w->sorted_homo.reserve(soff[Kv] * 3 * sizeof(float))))
    return rc;
  std::vector<SortItem> items(Kv);
  for (int j = 0; j < Kv; ++j)
    items[j] = SortItem{reinterpret_cast<const long long *>(w->user_samples[vk[j]].first), w->user_samples[vk[j]].second,
                        w->sorted_loc.as<long long>() + soff[j], w->sorted_homo.as<float>() + 3 * soff[j],
                        w->views[vk[j]].N};
  std::vector<int> status((size_t)2 * Kv, 0), tiles_nonempty(Kv, 0), pad_flags(Kv, 0);
  struct
  {
    DevBuf items, mark, status, tiles, pad;
  } d; // the relay's device temporaries (declared after the host vectors: released before they die)
  if ((rc = upload(d.items, items, w->stream)) || (rc = d.mark.reserve((size_t)Kv * HW * sizeof(int))) ||
      (rc = d.status.reserve((size_t)2 * Kv * sizeof(int))) || (rc = d.tiles.reserve((size_t)Kv * sizeof(int))))
    return rc;
  // walk order of the samples: image tiles of 8 x 8 pixels -- a wave's 64 consecutive samples then warp to a compact
  // footprint in every destination keyframe, which is what the LDS-staged sampler of the photometric linearize
  // needs (photo_kernels.hip).  SAGE_SAMPLE_TILE=WxH picks another tile, 0x0 the raster walk.
  static const std::pair<int, int> tile = [] {
    int tw = 8, th = 8;
    if (const char *e = getenv("SAGE_SAMPLE_TILE"))
      if (sscanf(e, "%dx%d", &tw, &th) != 2 || tw < 1 || th < 1)
        tw = th = 0;
    return std::make_pair(tw, th);
  }();
  SAGE_HIP(launch_sort_locations(w->stream, d.items.as<SortItem>(), Kv, max_n, HW, d.mark.as<int>(), d.status.as<int>(),
                                 (int)c.pyr.cam[0].w, tile.first, tile.second, nullptr, d.tiles.as<int>()));
  w->build_stats.ordered = Kv;
  w->build_stats.launches += max_n > 0 ? 4 : 3; // two fills, the mark pass, the ordering pass
  SAGE_HIP(hipMemcpyAsync(status.data(), d.status.p, status.size() * sizeof(int), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipMemcpyAsync(tiles_nonempty.data(), d.tiles.p, (size_t)Kv * sizeof(int), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  // r06 -- tile-padded order (producers.hip, order_locations_kernel): keyframes whose sampled tiles are not all full are relaid
  // with every sampled tile's 64 slots (holes = location -1), so that a wave of the kernels is one tile whatever the mask looks
  // like.  Only where it is cheap: slots <= 1.25 x samples (a dense mask with a ragged edge: a few percent; a sparse random
  // sample set would grow several-fold and keeps the compact order).  SAGE_SAMPLE_PAD=0 turns it off.
  bool any_pad = false;
  if (tile.first * tile.second == 64 && !(getenv("SAGE_SAMPLE_PAD") && atoi(getenv("SAGE_SAMPLE_PAD")) == 0))
    for (int j = 0; j < Kv; ++j)
    {
      const int n = w->views[vk[j]].N;
      const long long slots = 64ll * tiles_nonempty[j];
      if (status[2 * j] == 0 && status[2 * j + 1] == n && slots > n && 4 * slots <= 5ll * n)
      {
        pad_flags[j] = 1;
        any_pad = true;
      }
    }
  if (any_pad)
  {
    std::vector<int> status2((size_t)2 * Kv, 0);
    if ((rc = upload(d.pad, pad_flags, w->stream)))
      return rc;
    SAGE_HIP(launch_sort_locations(w->stream, d.items.as<SortItem>(), Kv, max_n, HW, d.mark.as<int>(), d.status.as<int>(),
                                   (int)c.pyr.cam[0].w, tile.first, tile.second, d.pad.as<int>(), nullptr, true));
    w->build_stats.launches += 1;
    SAGE_HIP(hipMemcpyAsync(status2.data(), d.status.p, status2.size() * sizeof(int), hipMemcpyDeviceToHost, w->stream));
    SAGE_HIP(hipStreamSynchronize(w->stream));
    for (int j = 0; j < Kv; ++j)
      if (pad_flags[j])
      {
        if (status2[2 * j + 1] != 64 * tiles_nonempty[j])
          return SAGE_E_STATE;
        w->views[vk[j]].N = status2[2 * j + 1]; // slots, holes included
      }
  }
  for (int j = 0; j < Kv; ++j)
  {
    const int k = vk[j];
    if (status[2 * j] > 0)
      return SAGE_E_INVALID; // a location outside the image
    if (status[2 * j + 1] != w->user_n[k])
      continue; // (a pixel sampled twice: the compaction dropped a sample -> keep the caller's order)
    w->views[k].loc1d = reinterpret_cast<const int64_t *>(items[j].loc_out);
    w->views[k].homo = items[j].homo_out;
  }
  return SAGE_OK;
}

// 5. leaves f0s: the pose-independent pre-sampled source features, once per keyframe; fs.f0s_off
static int finalize_source_features(SageWindow *w, FinalizeState &fs)
{
  const SageWindowConfig &c = w->cfg;
  const int FS = c.FS, K = w->K;
  int rc;
  // (a prepared keyframe brings its own: it takes no room here)
  fs.f0s_off.assign(K + 1, 0);
  for (int k = 0; k < K; ++k)
    fs.f0s_off[k + 1] = fs.f0s_off[k] + (w->prepared[k] ? 0 : (size_t)c.pyr.levels * FS * std::max(1, w->views[k].N));
  if ((rc = w->f0s.reserve(fs.f0s_off[K] * sizeof(float))))
    return rc;
  w->kf_f0s.assign(K, nullptr);
  for (int k = 0; k < K; ++k)
  {
    if (w->prepared[k])
    {
      w->kf_f0s[k] = w->prepared[k]->f0s;
      continue;
    }
    float *f0s = w->f0s.as<float>() + fs.f0s_off[k];
    SAGE_HIP(launch_presample_source(w->stream, f0s, w->kf_pk[k], w->views[k].homo, w->views[k].N, FS, c.pyr));
    w->kf_f0s[k] = f0s;
    w->build_stats.presampled += 1;
    w->build_stats.launches += w->views[k].N > 0 ? 1 : 0;
  }
  return SAGE_OK;
}

// 6. leaves n_edges, merge_ok, geo_px and the photometric / geometric edge tables of both variable sets; fs.px_off, fs.Nedge,
//    fs.adjv, fs.le and the residual / byte counts of the dense factors
static int finalize_edge_tables(SageWindow *w, FinalizeState &fs)
{
  const SageWindowConfig &c = w->cfg;
  const int CS = c.CS, FS = c.FS, K = w->K, HW = image_pixels(w);
  int rc;
  w->n_edges = (int)w->local_edges.size();
  // merged linearize (LaunchCommon::merge_geo_weight): the geometric kernel's per-pixel hand-over to the photometric one
  std::vector<size_t> &px_off = fs.px_off;
  px_off.assign((size_t)w->n_edges + 1, 0);
  for (int e = 0; e < w->n_edges; ++e)
  {
    const int ge = w->local_edges[e], l = ge / 2;
    const int k0 = ge % 2 == 0 ? w->links[l].first : w->links[l].second; // the source keyframe of the direction
    px_off[(size_t)e + 1] = px_off[e] + (size_t)std::max(1, w->views[k0].N);
  }
  w->merge_ok = c.use_photo && c.use_geo && c.geo_weight > 0.f && !sage::env_flag("SAGE_NO_MERGE");
  if (w->merge_ok)
  {
    if ((rc = w->geo_px.reserve(std::max<size_t>(1, px_off[w->n_edges]) * 4 * sizeof(float))))
      return rc;
    SAGE_HIP(hipMemsetAsync(w->geo_px.p, 0, std::max<size_t>(1, px_off[w->n_edges]) * 4 * sizeof(float), w->stream));
  }
  fs.le.assign(w->links.size(), LinkEdges{-1, -1});
  fs.Nedge.assign(w->n_edges, 0);
  fs.adjv.assign(K, std::vector<AdjEntry>());
  fs.residuals = fs.bytes = 0;
  const double rho = (double)c.pyr.P / (double)HW;
  for (int s = 0; s < 2; ++s)
  {
    std::vector<PhotoEdge> pt(w->n_edges);
    std::vector<GeoEdge> gt(w->n_edges);
    for (int e = 0; e < w->n_edges; ++e)
    {
      const int l = w->local_edges[e] / 2;
      const int ab[2] = {w->links[l].first, w->links[l].second};
      {
        const int dir = w->local_edges[e] % 2;
        const int k0 = ab[dir], k1 = ab[1 - dir];
        const SageKeyframeView &v0 = w->views[k0], &v1 = w->views[k1];
        const float *x0 = w->vars[s].as<float>() + (size_t)k0 * w->VS;
        const float *x1 = w->vars[s].as<float>() + (size_t)k1 * w->VS;
        PhotoEdge pe{};
        pe.feat0 = v0.feat_pyr; pe.feat1 = v1.feat_pyr; pe.grad1 = v1.grad_pyr; pe.bias0 = v0.bias;
        pe.feat0_pk = w->kf_pk[k0]; // (the window's own or the keyframe's handle's: stages 3 and 5)
        pe.feat1_pk = w->kf_pk[k1];
        pe.f0s = w->kf_f0s[k0];
        pe.dpt0 = w->dpt.as<float>() + (size_t)k0 * HW;
        pe.dpt1_geo = (c.use_photo && c.use_geo) ? w->dpt.as<float>() + (size_t)k1 * HW : nullptr;
        pe.geo_loss = w->link_geo_loss[l];
        pe.geo_px = w->merge_ok ? w->geo_px.as<float>() + 4 * px_off[e] : nullptr;
        pe.basis0 = v0.basis; pe.mask1 = c.mask_dev; pe.homo = v0.homo; pe.loc = v0.loc1d; pe.loc_is_i64 = 1;
        pe.R0 = x0; pe.t0 = x0 + 9; pe.R1 = x1; pe.t1 = x1 + 9; pe.R10 = nullptr; pe.t10 = nullptr;
        pe.code0 = x0 + 13; pe.scale0 = x0 + 12; pe.N = v0.N;
        pt[e] = pe;
        GeoEdge ge{};
        ge.dpt0 = w->dpt.as<float>() + (size_t)k0 * HW;
        ge.bias0 = v0.bias; ge.basis0 = v0.basis; ge.dpt1 = w->dpt.as<float>() + (size_t)k1 * HW;
        ge.dgrad1 = w->dgrad.as<float>() + (size_t)k1 * 2 * HW; ge.basis1 = v1.basis; ge.mask1 = c.mask_dev;
        ge.homo = v0.homo; ge.loc = v0.loc1d; ge.loc_is_i64 = 1;
        ge.R0 = x0; ge.t0 = x0 + 9; ge.R1 = x1; ge.t1 = x1 + 9; ge.R10 = nullptr; ge.t10 = nullptr;
        ge.code0 = x0 + 13; ge.scale0 = x0 + 12; ge.scale1 = x1 + 12; ge.N = v0.N;
        ge.loss_param = w->link_geo_loss[l];
        ge.px_out = w->merge_ok ? w->geo_px.as<float>() + 4 * px_off[e] : nullptr;
        gt[e] = ge;
        if (s == 0)
        {
          fs.Nedge[e] = v0.N;
          if (c.use_photo)
          {
            fs.adjv[k0].push_back(AdjEntry{0, e, 0});
            fs.adjv[k1].push_back(AdjEntry{0, e, 1});
            fs.residuals += (double)c.pyr.levels * w->user_n[k0] * FS; // (the caller's samples: holes of a padded order do not count)
            fs.bytes += (double)w->user_n[k0] * 4.0 * (4.0 * FS * rho + CS + 6.0);
          }
          if (c.use_geo)
          {
            fs.adjv[k0].push_back(AdjEntry{1, e, 0});
            fs.adjv[k1].push_back(AdjEntry{1, e, 1});
            fs.residuals += (double)w->user_n[k0];
            fs.bytes += (double)w->user_n[k0] * 4.0 * (2.0 * CS + 9.0);
          }
        }
      }
      if (s == 0)
        (w->local_edges[e] % 2 == 0 ? fs.le[l].e_ab : fs.le[l].e_ba) = e;
    }
    if ((rc = upload(w->dense[kPhoto].tab[s], pt, w->stream)) || (rc = upload(w->dense[kGeo].tab[s], gt, w->stream)))
      return rc;
    SAGE_HIP(hipStreamSynchronize(w->stream));
  }
  return SAGE_OK;
}

// 8. leaves the geometric and the photometric work list, Nedge and tpb_heur: the plan's run lengths, unless SAGE_GEO_TPB /
//    SAGE_PHOTO_TPB pin them.  The work items follow the order of the edges, an edge's runs one after the other:
// (r06, VERDICT r5 item 4 -- measured and dropped: the runs of an edge dealt to the XCDs in contiguous BANDS of image strips
//  (workgroup b runs on XCD b % 8; band x = runs [x R / 8, (x + 1) R / 8), all XCDs on the same edge at the same time), so that
//  vertically adjacent strips share their destination halo in ONE L2: config 4 photometric linearize 1.202 -> 1.191 ms, error
//  pass 0.638 -> 0.624, K = 64 unchanged (0.622 / 0.623) -- profiles/r06_kernel_ab_experiments.txt)
// (r05, VERDICT r4 item 6 -- measured and dropped: the linearize's work items in destination-keyframe-major order, the
//  runs of the <= 6 edges that sample one keyframe interleaved strip by strip, so that the workgroups in flight want ONE
//  packed pyramid at a time: config 4 photometric linearize 1.195 -> 1.356 ms, K = 64 0.677 -> 0.820 ms, config 2 0.157 ->
//  0.192 ms.  Consecutive runs of ONE edge share their source streams and overlap in the destination; the link order
//  (i-1,i) (i-2,i) (i-3,i), both directions adjacent, already keeps keyframe i in three of six consecutive edges.)
static int finalize_work_lists(SageWindow *w, const FinalizeState &fs)
{
  const std::vector<int> tiles = edge_tiles(fs.Nedge);
  int rc;
  int tpb_g = plan::geo_run(plan::total_tiles(tiles));
  if (const char *e = getenv("SAGE_GEO_TPB"))
    tpb_g = std::max(1, atoi(e));
  WorkList wl;
  wl.build(fs.Nedge, tpb_g);
  if ((rc = upload_work_list(w->dense[kGeo], wl, w->stream)))
    return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  int tpb = plan::photo_run(tiles, w->cfg.FS);
  if (const char *e = getenv("SAGE_PHOTO_TPB"))
    tpb = std::max(1, atoi(e));
  w->Nedge = fs.Nedge;
  w->tpb_heur = tpb;
  if ((rc = window_plan_photo_runs(w, tpb, photo_flush_for_runs(tpb))))
    return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  return SAGE_OK;
}

// 9. leaves the per-edge result buffers, the adjacency of the assembly, the ids of the blocks this rank assembles, the zeroed
//    packed system / error buffer and their host mirrors
static int finalize_results(SageWindow *w, const FinalizeState &fs)
{
  const int CS = w->cfg.CS, K = w->K;
  int rc;
  const size_t ne = std::max(1, w->n_edges);
  DenseSide &ph = w->dense[kPhoto], &ge = w->dense[kGeo];
  if ((rc = ph.reserve_results(ne, dense_dim(kPhoto, CS), std::max(ph.n_work, w->photo_rec.n), photo_partial_floats(CS))) ||
      (rc = ge.reserve_results(ne, dense_dim(kGeo, CS), ge.n_work, geo_partial_floats(CS))))
    return rc;
  // adjacency for the assembly
  std::vector<int32_t> adj_start(K + 1, 0);
  std::vector<AdjEntry> adj;
  for (int k = 0; k < K; ++k)
  {
    adj_start[k] = (int32_t)adj.size();
    adj.insert(adj.end(), fs.adjv[k].begin(), fs.adjv[k].end());
  }
  adj_start[K] = (int32_t)adj.size();
  if ((rc = upload(w->adj_start, adj_start, w->stream)) || (rc = upload(w->adj, adj, w->stream)) ||
      (rc = upload(w->link_edges, fs.le, w->stream)))
    return rc;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  if ((rc = w->packed.reserve(sage_window_packed_count(w) * sizeof(double))) || (rc = w->errbuf.reserve(4 * sizeof(double))))
    return rc;
  {
    // the output blocks this rank's edges and keypoint terms contribute to (everything, on a single-rank window; a link block
    // that only local terms write to is listed too: it would keep the zeros of this stage on a sharded window)
    // (... and so is a block a local prior term adds to: prior_add_kernel adds to what the assembly wrote)
    std::vector<int32_t> ids;
    const std::vector<int> &pb = w->priors.layout.blocks;
    auto prior_block = [&pb](int id) { return std::binary_search(pb.begin(), pb.end(), id); };
    for (int k = 0; k < K; ++k)
      if (!fs.adjv[k].empty() || prior_block(k))
        ids.push_back(k);
    for (size_t l = 0; l < fs.le.size(); ++l)
      if (fs.le[l].e_ab >= 0 || fs.le[l].e_ba >= 0 || fs.link_terms[l] || prior_block(K + (int)l))
        ids.push_back(K + (int32_t)l);
    ids.push_back(K + (int32_t)w->links.size()); // the tail
    w->dist.n_asm_blocks = (int)ids.size();
    if ((rc = upload(w->dist.asm_blocks, ids, w->stream)))
      return rc;
    SAGE_HIP(hipStreamSynchronize(w->stream));
  }
  SAGE_HIP(hipMemsetAsync(w->packed.p, 0, sage_window_packed_count(w) * sizeof(double), w->stream));
  SAGE_HIP(hipMemsetAsync(w->errbuf.p, 0, 4 * sizeof(double), w->stream));
  if (!w->mirror.h)
  {
    if ((rc = w->mirror.mem.reserve(TotalsMirror::kDoubles * sizeof(double))))
      return rc;
    w->mirror.h = w->mirror.mem.as<double>();
    std::memset(w->mirror.h, 0, TotalsMirror::kDoubles * sizeof(double));
  }
  w->host_packed.assign(sage_window_packed_count(w), 0.0);
  w->delta.assign((size_t)K * w->B, 0.0);
  return SAGE_OK;
}

// 10. leaves the device solver (none for duplicate links: the host block solve) and, for a window of the domain-decomposed
//     solve, the shard plan with its separator buffers
static int finalize_solver(SageWindow *w, const FinalizeState &fs)
{
  int rc = solver_create(&w->solver, w->K, w->rows, w->VS, w->links, w->stream);
  if (rc != SAGE_OK && rc != SAGE_E_UNSUPPORTED)
    return rc;
  if (w->solver && window_has_holds(w) && (rc = solver_set_holds(w->solver, w->hold, w->stream)))
    return rc; // (without a device solver the host block solve masks its copy: window_solve.hip)
  if (!fs.domain_solve)
    return SAGE_OK;
  const std::vector<int32_t> lk = window_link_pairs(w);
  if ((rc = sage_shard_plan_create(w->K, (int)w->links.size(), lk.data(), w->B, w->rank, w->world, &w->dist.shard)))
    return rc;
  const size_t ns = sage_shard_sep_count(w->dist.shard);
  w->dist.h_sep.assign(ns, 0.0);
  if ((rc = w->dist.sepbuf.reserve(ns * sizeof(double))))
    return rc;
  w->host_packed.resize(sage_window_packed_count(w));
  return SAGE_OK;
}

extern "C" int sage_window_finalize(SageWindow *w)
{
  if (!w || w->finalized || w->K < 1)
    return SAGE_E_INVALID;
  FinalizeState fs;
  const char *schur = getenv("SAGE_SHARD_SCHUR"); // the request: 0 / 1
  fs.domain_solve = plan::uses_domain_solve(w->world, w->K, schur ? atoi(schur) != 0 : -1);
  w->hold.resize(w->K, 0);
  if (fs.domain_solve && (window_has_holds(w) || !w->terms.gt_added.empty() || !w->priors.added.empty()))
    return SAGE_E_UNSUPPORTED; // (the domain-decomposed solve knows no held variables, no term on a single keyframe, no prior term)
  w->rows = plan::solver_rows(w->hold.data(), w->K, w->cfg.CS);
  w->build_stats = SageWindowBuildStats{};
  w->build_stats.keyframes = w->K;
  w->build_stats.prepared = w->K - (int)std::count(w->prepared.begin(), w->prepared.end(), nullptr);
  int rc;
  if ((rc = finalize_variables(w)) || (rc = finalize_ownership(w, fs)) || (rc = finalize_pyramids(w)) ||
      (rc = finalize_samples(w)) || (rc = finalize_source_features(w, fs)) || (rc = finalize_edge_tables(w, fs)) ||
      (rc = finalize_terms(w, fs)) || (rc = finalize_priors(w)))
    return rc;
  w->residuals_per_lin = fs.residuals;
  w->bytes_per_lin = fs.bytes;
  if ((rc = finalize_work_lists(w, fs)) || (rc = finalize_results(w, fs)) || (rc = finalize_solver(w, fs)))
    return rc;
  w->finalized = true;
  if (const char *e = getenv("SAGE_AUTOTUNE")) // 11. optional: time the run lengths on the window itself
    if (atoi(e) != 0)
      return sage_window_tune_runs(w, nullptr, nullptr, nullptr, nullptr);
  return SAGE_OK;
}

// the run length a previous sage_window_tune_runs found for this window geometry (an embedder tunes once per image size / mask / window
// length and re-applies the result to the windows it builds afterwards: the tuning costs 20-40 ms, a window lives for a few LM steps).
// A system assembled before the call belongs to the previous plan and is dropped: a linearize must follow (sage_window_lm_step
// does its own; sage_window_solve answers SAGE_E_STATE until then), so that results stay bit-reproducible for the run length
extern "C" int sage_window_set_runs(SageWindow *w, int tpb)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  if (tpb < 1 || tpb > 64)
    return SAGE_E_INVALID;
  const int rc = window_plan_photo_runs(w, tpb, photo_flush_for_runs(tpb));
  window_invalidate_plan_results(w);
  return rc;
}

// r06 -- run-length tuning of the photometric kernels, measured on the window itself.  The time of the photometric linearize
// and of the error pass depends on the run length of a workgroup in a way no static rule captured (profiles/
// r06_kernel_ab_experiments.txt s16): which runs share an XCD's L2 with which, how run boundaries fall on image strips, how the
// workgroups fill the 768 slots.  On BASELINE config 4 runs of 12 are 6 % faster than the rule's 8 while 11 and 13 are 14 % slower; on
// a 192 x 256 window the rule's 8 is strip-aligned and 18 % (error pass: 27 %) slower than 6.  This call times the candidates on
// the window's own data -- three timed linearize + error-pass evaluations each at the current estimate, the rule measured first and last -- and keeps the fastest if it beats
// the rule's choice by >= 4 % (so that equal candidates do not flip between calls: results are bit-reproducible for a given run
// length, not across run lengths).  Opt-in: an explicit call, or SAGE_AUTOTUNE=1 at sage_window_finalize; SAGE_PHOTO_TPB pins
// the run length and disables it.  Single-rank windows only (a sharded window's linearize contains a collective).
// The timed evaluations leave `packed` assembled under whichever plan was measured last, not necessarily the one kept: it is
// dropped at the end, and a linearize must follow (as after sage_window_set_runs).
extern "C" int sage_window_tune_runs(SageWindow *w, int *tpb_out, int *tpb_rule_out, float *ms_rule_out, float *ms_best_out)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  const int rule = w->tpb_heur;
  if (tpb_out)
    *tpb_out = w->dense[kPhoto].tpb;
  if (tpb_rule_out)
    *tpb_rule_out = rule;
  if (ms_rule_out)
    *ms_rule_out = 0.f;
  if (ms_best_out)
    *ms_best_out = 0.f;
  if (getenv("SAGE_PHOTO_TPB") || w->world > 1 || w->dist.allreduce || w->n_edges == 0 || !(w->cfg.use_photo))
    return SAGE_OK;
  const std::vector<int> cand = plan::tune_candidates(rule, plan::typical_edge(edge_tiles(w->Nedge)));
  const bool prof_was = w->prof.profiling;
  const int level_was = w->prof.prof_level;
  const int relin_was = w->relin.mode; // every timed linearize evaluates every edge
  w->relin.mode = SAGE_RELIN_ALL;
  int rc = sage_window_set_profiling(w, 1);
  double best_ms = 0.0, rule_ms = 0.0;
  int best = rule;
  // one plan's time: an untimed evaluation (its caches), then the fastest of three
  auto measure = [&](int t, double &ms) -> int {
    int r = window_plan_photo_runs(w, t, photo_flush_for_runs(t));
    for (int rep = 0; rep < 4 && !r; ++rep)
    {
      if ((r = sage_window_linearize(w)) || (r = sage_window_error(w, 1)))
        break;
      double lin = 0.0, err = 0.0;
      int nl = 0, ne = 0;
      if ((r = sage_window_get_kernel_time(w, 0, &lin, &nl)) || (r = sage_window_get_kernel_time(w, 2, &err, &ne)))
        break;
      const double tt = lin / std::max(1, nl) + err / std::max(1, ne);
      if (rep > 0)
        ms = rep == 1 ? tt : std::min(ms, tt);
    }
    return r;
  };
  // the device's clocks and caches settle over the first ~25 evaluations of a process (profiles/r04_step_series.txt): the rule's plan
  // is measured first AND last, so that whoever comes first is not charged for the warm-up
  for (int i = 0; i < 8 && !rc; ++i)
    if ((rc = sage_window_linearize(w)) || (rc = sage_window_error(w, 1)))
      break;
  (void)sage_window_get_kernel_time(w, 0, nullptr, nullptr);
  (void)sage_window_get_kernel_time(w, 2, nullptr, nullptr);
  if (!rc)
    rc = measure(rule, rule_ms);
  best_ms = rule_ms;
  for (size_t c = 1; c < cand.size() && !rc; ++c)
  {
    double ms = 0.0;
    if ((rc = measure(cand[c], ms)))
      break;
    if (ms < best_ms)
    {
      best_ms = ms;
      best = cand[c];
    }
  }
  if (!rc && best != rule)
  {
    double again = 0.0;
    if (!(rc = measure(rule, again)))
      rule_ms = std::min(rule_ms, again);
  }
  (void)sage_window_get_kernel_time(w, 1, nullptr, nullptr); // (drop the geometric kernels' records of these evaluations)
  (void)sage_window_get_kernel_time(w, 3, nullptr, nullptr);
  (void)sage_window_set_profiling(w, prof_was ? level_was : 0);
  w->relin.mode = relin_was;
  if (!rc && !(best_ms < 0.96 * rule_ms))
    best = rule;
  const int rc2 = window_plan_photo_runs(w, rc ? rule : best, photo_flush_for_runs(rc ? rule : best));
  window_invalidate_plan_results(w);
  if (tpb_out)
    *tpb_out = w->dense[kPhoto].tpb;
  if (ms_rule_out)
    *ms_rule_out = (float)rule_ms;
  if (ms_best_out)
    *ms_best_out = (float)(best == rule ? rule_ms : best_ms);
  return rc ? rc : rc2;
}
