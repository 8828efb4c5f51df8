// tracker.hip -- sage_track_frame: the tracker's LM callbacks wired to the HIP operators (camera_tracker.cpp:1034-1672).
#include "runtime_internal.h"

// =====================================================================================================
// tracker: product wiring of the LM callbacks to the HIP kernels
// =====================================================================================================
namespace
{
struct TrackCtx
{
  const SageTrackProblem *prob;
  int dof;
};

// depths the kernels of one evaluation read: dof 6 -> the caller's metric depths; dof 7 -> scale * unscaled
// (camera_tracker.cpp:264, :273 candidate error; :431, :453 Jacobian)
int track_depths(TrackCtx *c, float scale, const float **photo, const float **kp)
{
  const SageTrackProblem *p = c->prob;
  SageWorkspace *ws = p->ws;
  *photo = p->dpts0_dev;
  *kp = p->kp_dpts0_dev;
  if (c->dof != 7)
    return 0;
  hipStream_t s = ws->stream;
  if (p->use_photo)
  {
    SAGE_HIP(launch_scale_array(s, ws->trk_dpts.as<float>(), p->dpts0_dev, scale, p->N));
    *photo = ws->trk_dpts.as<float>();
  }
  if (p->use_keypoints)
  {
    SAGE_HIP(launch_scale_array(s, ws->trk_kp_dpts.as<float>(), p->kp_dpts0_dev, scale, p->NK));
    *kp = ws->trk_kp_dpts.as<float>();
  }
  return 0;
}

// One evaluation of the tracker's cost at (pose, scale): CameraTracker::ComputeJacobianAndError (camera_tracker.cpp:282-328
// dof 6, :330-374 dof 7) with jac, CameraTracker::ComputeError (:220-248 dof 6, :250-280 dof 7) without.
// Zero-copy (r04): the kernels read the pose straight from the pinned TrackHost and write both terms' AtA / Atb /
// statistics straight into it; a one-lane kernel posts a ticket behind them and the host spins on it (ws_ticket_wait).  Per
// evaluation this replaces a host-to-device copy, a device-to-host copy and a blocking hipStreamSynchronize (each a 5-10 us
// round trip through the runtime) by two PCIe accesses of the kernels themselves (the reference pays a .item() synchronise
// per term and three more in each term's host reduction)
int track_eval(TrackCtx *c, const float *pose12, float scale, bool jac, float *AtA, float *Atb, float *error)
{
  const SageTrackProblem *p = c->prob;
  SageWorkspace *ws = p->ws;
  const int dof = c->dof;
  TrackHost *h = ws->trk();
  std::memcpy(h->pose, pose12, sizeof(h->pose)); // (the previous evaluation has been waited for: nobody reads it)
  const float *R = h->pose, *t = R + 9;          // (pinned, device-visible)
  const float *dp, *kdp;
  int rc;
  if ((rc = track_depths(c, scale, &dp, &kdp)))
    return rc;
  float *st_photo = h->stats, *st_kp = h->stats + 2;
  // (the error variants: no outputs, no gradient, and depths that carry the scale already)
  if (p->use_photo &&
      (rc = track_photo_enqueue(ws, jac, jac ? dof : 6, jac ? h->photo_AtA : nullptr, jac ? h->photo_Atb : nullptr, st_photo, R,
                                t, p->mask1_dev, dp, p->homo_dev, p->feat0s_dev, p->feat1_dev, jac ? p->grad1_dev : nullptr,
                                &p->pyr, jac ? scale : 1.0f, p->eps, p->weights_dev, p->N, p->FS)))
    return rc;
  if (p->use_keypoints)
  {
    float *kA = jac ? h->kp_AtA : nullptr, *kb = jac ? h->kp_Atb : nullptr;
    if (dof == 6)
      rc = track_reproj_enqueue(ws, jac, kA, kb, st_kp, R, t, kdp, p->kp_homo0_dev, p->kp_matched_2d_dev, &p->pyr.cam[0],
                                p->eps, p->kp_loss_param, p->kp_weight, p->NK);
    else
      rc = track_match_geom_enqueue(ws, jac ? 3 : 2, jac, kA, kb, st_kp, R, t, kdp, p->kp_matched_dpts1_dev, p->kp_homo0_dev,
                                    p->kp_matched_homo1_dev, jac ? scale : 1.f, p->kp_loss_param, p->kp_weight, p->NK);
    if (rc)
      return rc;
  }
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  const float e_photo = p->use_photo ? st_photo[0] : 0.f, e_kp = p->use_keypoints ? st_kp[0] : 0.f;
  if (jac)
  {
    // AtA = zeros; AtA += photo_AtA; AtA += keypoint_AtA  (fp32 tensor adds, :296-318 / :344-364)
    for (int i = 0; i < dof * dof; ++i)
      AtA[i] = (p->use_photo ? 0.f + h->photo_AtA[i] : 0.f) + (p->use_keypoints ? h->kp_AtA[i] : 0.f);
    for (int i = 0; i < dof; ++i)
      Atb[i] = (p->use_photo ? 0.f + h->photo_Atb[i] : 0.f) + (p->use_keypoints ? h->kp_Atb[i] : 0.f);
  }
  *error = e_photo + e_kp;
  return 0;
}

int track_lin_cb(void *vctx, const float *pose12, float scale, float *AtA, float *Atb, float *error)
{
  return track_eval(static_cast<TrackCtx *>(vctx), pose12, scale, true, AtA, Atb, error);
}

int track_err_cb(void *vctx, const float *pose12, float scale, float *error)
{
  return track_eval(static_cast<TrackCtx *>(vctx), pose12, scale, false, nullptr, nullptr, error);
}

// what sage_track_frame and sage_track_frame_batch ask of one problem (dof is 6 or 7)
bool track_problem_valid(int dof, const SageTrackProblem *prob)
{
  if (!prob || !prob->ws)
    return false;
  if (!prob->use_photo && !prob->use_keypoints) // "at least one factor should be enabled" (camera_tracker.cpp:1328)
    return false;
  if (prob->use_photo && (!prob->mask1_dev || !prob->dpts0_dev || !prob->homo_dev || !prob->feat0s_dev ||
                          !prob->feat1_dev || !prob->grad1_dev || !prob->weights_dev || prob->N < 1))
    return false;
  if (prob->use_keypoints &&
      (!prob->kp_dpts0_dev || !prob->kp_homo0_dev || prob->NK < 1 ||
       (dof == 6 ? !prob->kp_matched_2d_dev : (!prob->kp_matched_dpts1_dev || !prob->kp_matched_homo1_dev))))
    return false;
  return true;
}
} // namespace

extern "C" int sage_track_frame(const SageLmConfig *cfg, int dof, const SageTrackProblem *prob, float *pose12,
                                float *scale, float *final_error, int *iters, SageLmTraceEntry *trace, int trace_cap,
                                int *trace_len)
{
  if (!cfg || !pose12 || (dof != 6 && dof != 7) || (dof == 7 && !scale) || !track_problem_valid(dof, prob))
    return SAGE_E_INVALID;
  TrackCtx ctx;
  ctx.prob = prob;
  ctx.dof = dof;
  SageWorkspace *ws = prob->ws;
  int rc;
  // evaluation buffers of the workspace: allocated once, reused by every frame tracked through it
  if (!ws->trk_host.p)
  {
    if ((rc = ws->trk_host.reserve(sizeof(TrackHost))))
      return rc;
    std::memset(ws->trk(), 0, sizeof(TrackHost));
  }
  if (dof == 7 && ((prob->use_photo && (rc = ws->trk_dpts.reserve((size_t)prob->N * sizeof(float)))) ||
                   (prob->use_keypoints && (rc = ws->trk_kp_dpts.reserve((size_t)prob->NK * sizeof(float))))))
    return rc;
  return sage_track_lm(cfg, dof, track_lin_cb, track_err_cb, &ctx, pose12, scale, final_error, iters, trace, trace_cap,
                       trace_len);
}


// =====================================================================================================
// batched tracker: B problems in lock-step (sage_track_lm_batch), one round = one evaluation of every live problem
// =====================================================================================================
// dof 7 first forms the depths of the round, scale * unscaled, for every problem and term in ONE launch into the problems'
// slices of a scratch array (the single call's scale passes, batched: forming the product inside the kernels changed how
// the compiler fuses the multiply-adds around it and with that single bits of the results).  Then, per
// round and kind of request (linearize / error-only: different kernels), one photometric launch over the (problem, tile)
// items of the problems that asked for it, with one finalize workgroup per problem, and one keypoint launch with a workgroup
// per problem; then ONE ticket.  Everything a kernel reads about a problem comes from the call's pinned tables (TrackHost
// [B]: poses in, results out; TrackBatchProblem / KpTrackProblem [B]; the round's items and request lists): the host writes
// them between the ticket of one round and the launches of the next, no copy is enqueued.  Row b of a batch is the single
// call's result bit for bit: the same per-pixel body and keypoint contraction, the records of a problem summed in tile order.
namespace
{
struct TrackBatchCtx
{
  const SageTrackProblem *probs = nullptr;
  SageWorkspace *ws = nullptr;
  int B = 0, dof = 6;
  // pinned (ws->trk_table)
  TrackBatchProblem *photo = nullptr;
  KpTrackProblem *kp = nullptr;
  WorkItem *work[2] = {nullptr, nullptr};  // [jac]: the round's items
  int32_t *req[2] = {nullptr, nullptr};    // [jac]: the round's photometric requests
  int32_t *kp_req[2] = {nullptr, nullptr}; // [jac]: the round's keypoint requests on the batched launch
  ScaleBatchItem *scale_items = nullptr;   // the round's scale pass (dof 7): up to two arrays per problem
  int n_tiles[SAGE_TRACK_MAX_BATCH];
  size_t kp_lds[SAGE_TRACK_MAX_BATCH]; // 0: the rows do not fit one workgroup's LDS -> the single call's launches
};

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
bool ctx_kp_fits(int rpp, int NK, int D) { return kp_small_lds_bytes(rpp, NK, D) <= kKpSmallLdsMax; }

// the keypoint term of ONE problem through the single call's launches (rows past the one-workgroup LDS budget), results
// into the problem's TrackHost: what track_eval enqueues
int track_batch_kp_fallback(TrackBatchCtx *c, int b, bool jac, float scale)
{
  const SageTrackProblem *p = &c->probs[b];
  SageWorkspace *ws = c->ws;
  TrackHost *h = ws->trk() + b;
  const float *R = h->pose, *t = R + 9;
  const float *kdp = p->kp_dpts0_dev;
  if (c->dof == 7)
  {
    SAGE_HIP(launch_scale_array(ws->stream, ws->trk_kp_dpts.as<float>(), p->kp_dpts0_dev, scale, p->NK));
    kdp = ws->trk_kp_dpts.as<float>();
  }
  float *kA = jac ? h->kp_AtA : nullptr, *kb = jac ? h->kp_Atb : nullptr;
  if (c->dof == 6)
    return track_reproj_enqueue(ws, jac, kA, kb, h->stats + 2, R, t, kdp, p->kp_homo0_dev, p->kp_matched_2d_dev, &p->pyr.cam[0],
                                p->eps, p->kp_loss_param, p->kp_weight, p->NK);
  return track_match_geom_enqueue(ws, jac ? 3 : 2, jac, kA, kb, h->stats + 2, R, t, kdp, p->kp_matched_dpts1_dev, p->kp_homo0_dev,
                                  p->kp_matched_homo1_dev, jac ? scale : 1.f, p->kp_loss_param, p->kp_weight, p->NK);
}

int track_batch_eval(void *vctx, int n, const int32_t *problem, const int32_t *want_jac, const float *pose12, const float *scale,
                     float *AtA, float *Atb, float *error)
{
  TrackBatchCtx *c = static_cast<TrackBatchCtx *>(vctx);
  SageWorkspace *ws = c->ws;
  const SageTrackProblem &p0 = c->probs[0]; // (FS, use_*, eps and pyr are the batch's)
  const int dof = c->dof;
  int n_work[2] = {0, 0}, n_req[2] = {0, 0}, n_kp[2] = {0, 0}, n_scale = 0, max_scale_n = 0;
  size_t kp_lds[2] = {0, 0};
  for (int i = 0; i < n; ++i)
  {
    const int b = problem[i], j = want_jac[i] ? 1 : 0;
    const float s = scale[i];
    std::memcpy(ws->trk()[b].pose, pose12 + 12 * (size_t)i, 12 * sizeof(float)); // (the last round has been waited for)
    if (p0.use_photo)
    {
      c->photo[b].E.scale0 = j ? s : 1.0f;
      if (dof == 7)
      {
        c->scale_items[n_scale++] = ScaleBatchItem{c->probs[b].dpts0_dev, const_cast<float *>(c->photo[b].E.dpts0), s, c->probs[b].N};
        max_scale_n = std::max(max_scale_n, (int)c->probs[b].N);
      }
      c->req[j][n_req[j]++] = b;
      for (int t = 0; t < c->n_tiles[b]; ++t)
        c->work[j][n_work[j]++] = WorkItem{b, t};
    }
    if (p0.use_keypoints && c->kp_lds[b])
    {
      c->kp[b].scale0 = s;
      if (dof == 7)
      {
        c->scale_items[n_scale++] = ScaleBatchItem{c->probs[b].kp_dpts0_dev, const_cast<float *>(c->kp[b].dpts0), s, c->probs[b].NK};
        max_scale_n = std::max(max_scale_n, (int)c->probs[b].NK);
      }
      c->kp_req[j][n_kp[j]++] = b;
      kp_lds[j] = std::max(kp_lds[j], c->kp_lds[b]);
    }
  }
  SAGE_HIP(launch_scale_batch(ws->stream, c->scale_items, n_scale, max_scale_n));
  TrackBatchParams tp{};
  tp.probs = c->photo;
  tp.partials = ws->trk_bpart.as<float>();
  tp.pyr = p0.pyr;
  tp.eps = p0.eps;
  for (int j = 1; j >= 0; --j)
  {
    if (n_req[j])
    {
      tp.work = c->work[j];
      tp.requests = c->req[j];
      tp.dof = j ? dof : 6;
      SAGE_HIP(launch_track_batch(ws->stream, j != 0, p0.FS, tp, n_work[j], n_req[j]));
    }
    if (n_kp[j])
      SAGE_HIP(launch_kp_track_batch(ws->stream, dof, j != 0, c->kp, c->kp_req[j], n_kp[j], kp_lds[j], p0.pyr.cam[0], p0.eps));
  }
  int rc;
  if (p0.use_keypoints)
    for (int i = 0; i < n; ++i)
      if (!c->kp_lds[problem[i]] && (rc = track_batch_kp_fallback(c, problem[i], want_jac[i] != 0, scale[i])))
        return rc;
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  // AtA = photo + keypoints, Atb, error per problem: track_eval's fp32 sums, in its order
  for (int i = 0; i < n; ++i)
  {
    const TrackHost *h = ws->trk() + problem[i];
    const float e_photo = p0.use_photo ? h->stats[0] : 0.f, e_kp = p0.use_keypoints ? h->stats[2] : 0.f;
    if (want_jac[i])
    {
      float *A = AtA + 49 * (size_t)i, *g = Atb + 7 * (size_t)i;
      for (int k = 0; k < dof * dof; ++k)
        A[k] = (p0.use_photo ? 0.f + h->photo_AtA[k] : 0.f) + (p0.use_keypoints ? h->kp_AtA[k] : 0.f);
      for (int k = 0; k < dof; ++k)
        g[k] = (p0.use_photo ? 0.f + h->photo_Atb[k] : 0.f) + (p0.use_keypoints ? h->kp_Atb[k] : 0.f);
    }
    error[i] = e_photo + e_kp;
  }
  return 0;
}

bool same_pyramid(const SagePyramid &a, const SagePyramid &b)
{
  if (a.levels != b.levels || a.P != b.P)
    return false;
  for (int l = 0; l < a.levels && l < SAGE_MAX_LEVELS; ++l)
    if (a.level_offsets[l] != b.level_offsets[l] || std::memcmp(&a.cam[l], &b.cam[l], sizeof(SageCamera)) != 0)
      return false;
  return true;
}
} // namespace

extern "C" int sage_track_frame_batch(const SageLmConfig *cfg, int dof, const SageTrackProblem *probs, int B, float *pose12,
                                      float *scale, float *final_error, int *iters, int *status, SageLmTraceEntry *trace,
                                      int trace_cap, int *trace_len)
{
  if (!cfg || !pose12 || !status || (dof != 6 && dof != 7) || (dof == 7 && !scale) || B < 0 || B > SAGE_TRACK_MAX_BATCH)
    return SAGE_E_INVALID;
  if (B == 0)
    return SAGE_OK;
  if (!probs)
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
  {
    const SageTrackProblem &p = probs[b], &p0 = probs[0];
    if (!track_problem_valid(dof, &p))
      return SAGE_E_INVALID;
    if (p.ws != p0.ws || p.FS != p0.FS || !p.use_photo != !p0.use_photo || !p.use_keypoints != !p0.use_keypoints ||
        std::memcmp(&p.eps, &p0.eps, sizeof(float)) != 0 || !same_pyramid(p.pyr, p0.pyr))
      return SAGE_E_INVALID;
  }
  const SageTrackProblem &p0 = probs[0];
  if (p0.use_photo && ((p0.FS != 16 && p0.FS != 32) || p0.pyr.levels < 1 || p0.pyr.levels > SAGE_MAX_LEVELS))
    return SAGE_E_UNSUPPORTED; // (what the single call's photometric operator answers)
  SageWorkspace *ws = p0.ws;
  TrackBatchCtx ctx;
  ctx.probs = probs;
  ctx.ws = ws;
  ctx.B = B;
  ctx.dof = dof;
  // the call's buffers: TrackHost [B], the tables, the partial records; allocated once, grown when a batch needs more
  int rc;
  if (ws->trk_host.cap < (size_t)B * sizeof(TrackHost))
  {
    if ((rc = ws->trk_host.reserve((size_t)B * sizeof(TrackHost))))
      return rc;
    std::memset(ws->trk(), 0, ws->trk_host.cap);
  }
  long long total_tiles = 0, total_depths = 0;
  int max_fallback_nk = 0;
  const int rpp = dof == 6 ? kReprojRows : kMgRows;
  for (int b = 0; b < B; ++b)
  {
    ctx.n_tiles[b] = p0.use_photo ? (probs[b].N + kTile - 1) / kTile : 0;
    total_tiles += ctx.n_tiles[b];
    if (dof == 7)
      total_depths += (p0.use_photo ? probs[b].N : 0) + (p0.use_keypoints && ctx_kp_fits(rpp, probs[b].NK, dof) ? probs[b].NK : 0);
    const size_t lds = p0.use_keypoints ? kp_small_lds_bytes(rpp, probs[b].NK, dof) : 0; // (impl()'s own test)
    ctx.kp_lds[b] = lds <= kKpSmallLdsMax ? lds : 0;
    if (p0.use_keypoints && !ctx.kp_lds[b])
      max_fallback_nk = std::max(max_fallback_nk, probs[b].NK);
  }
  const size_t o_photo = 0, o_kp = align16(o_photo + (size_t)B * sizeof(TrackBatchProblem));
  const size_t o_req = align16(o_kp + (size_t)B * sizeof(KpTrackProblem));
  const size_t o_items = align16(o_req + 4 * (size_t)SAGE_TRACK_MAX_BATCH * sizeof(int32_t));
  const size_t o_work = align16(o_items + 2 * (size_t)B * sizeof(ScaleBatchItem));
  const size_t work_bytes = align16((size_t)std::max<long long>(total_tiles, 1) * sizeof(WorkItem));
  if ((rc = ws->trk_table.reserve(o_work + 2 * work_bytes)) ||
      (rc = ws->trk_bpart.reserve((size_t)std::max<long long>(total_tiles, 1) * kTrackScalars * sizeof(float))) ||
      (total_depths && (rc = ws->trk_bdpts.reserve((size_t)total_depths * sizeof(float)))) ||
      (dof == 7 && max_fallback_nk && (rc = ws->trk_kp_dpts.reserve((size_t)max_fallback_nk * sizeof(float)))))
    return rc;
  char *tab = ws->trk_table.as<char>();
  ctx.photo = reinterpret_cast<TrackBatchProblem *>(tab + o_photo);
  ctx.kp = reinterpret_cast<KpTrackProblem *>(tab + o_kp);
  ctx.scale_items = reinterpret_cast<ScaleBatchItem *>(tab + o_items);
  float *depths = ws->trk_bdpts.as<float>(); // dof 7: the next free slice of the round's scaled depths
  for (int j = 0; j < 2; ++j)
  {
    ctx.req[j] = reinterpret_cast<int32_t *>(tab + o_req) + (size_t)j * SAGE_TRACK_MAX_BATCH;
    ctx.kp_req[j] = reinterpret_cast<int32_t *>(tab + o_req) + (size_t)(2 + j) * SAGE_TRACK_MAX_BATCH;
    ctx.work[j] = reinterpret_cast<WorkItem *>(tab + o_work + (size_t)j * work_bytes);
  }
  int first = 0;
  for (int b = 0; b < B; ++b)
  {
    const SageTrackProblem &p = probs[b];
    TrackHost *h = ws->trk() + b;
    TrackBatchProblem tb{};
    if (p0.use_photo)
    {
      tb.E.feat0s = p.feat0s_dev; tb.E.feat1 = p.feat1_dev; tb.E.grad1 = p.grad1_dev; tb.E.mask1 = p.mask1_dev;
      tb.E.homo = p.homo_dev; tb.E.dpts0 = dof == 7 ? depths : p.dpts0_dev; tb.E.R = h->pose; tb.E.t = h->pose + 9; tb.E.weights = p.weights_dev;
      tb.E.scale0 = 1.0f; tb.E.N = p.N;
      tb.n_tiles = ctx.n_tiles[b]; tb.partial_first = first;
      if (dof == 7)
        depths += p.N;
      tb.AtA = h->photo_AtA; tb.Atb = h->photo_Atb; tb.stats = h->stats;
      first += ctx.n_tiles[b];
    }
    ctx.photo[b] = tb;
    KpTrackProblem kb{};
    if (p0.use_keypoints)
    {
      kb.R = h->pose; kb.t = h->pose + 9; kb.dpts0 = dof == 7 && ctx.kp_lds[b] ? depths : p.kp_dpts0_dev; kb.homo0 = p.kp_homo0_dev;
      if (dof == 7 && ctx.kp_lds[b])
        depths += p.NK;
      kb.matched_2d = p.kp_matched_2d_dev; kb.dpts1 = p.kp_matched_dpts1_dev; kb.homo1 = p.kp_matched_homo1_dev;
      kb.scale0 = 1.0f; kb.loss_param = p.kp_loss_param; kb.weight = p.kp_weight; kb.N = p.NK; kb.loss = SAGE_LOSS_FAIR;
      kb.AtA = h->kp_AtA; kb.Atb = h->kp_Atb; kb.stats = h->stats + 2;
    }
    ctx.kp[b] = kb;
  }
  return sage_track_lm_batch(cfg, dof, B, track_batch_eval, &ctx, pose12, scale, final_error, iters, status, trace, trace_cap,
                             trace_len);
}
