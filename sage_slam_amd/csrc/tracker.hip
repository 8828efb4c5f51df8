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
} // namespace

extern "C" int sage_track_frame(const SageLmConfig *cfg, int dof, const SageTrackProblem *prob, float *pose12,
                                float *scale, float *final_error, int *iters, SageLmTraceEntry *trace, int trace_cap,
                                int *trace_len)
{
  if (!cfg || !prob || !prob->ws || !pose12 || (dof != 6 && dof != 7) || (dof == 7 && !scale))
    return SAGE_E_INVALID;
  if (!prob->use_photo && !prob->use_keypoints) // "at least one factor should be enabled" (camera_tracker.cpp:1328)
    return SAGE_E_INVALID;
  if (prob->use_photo && (!prob->mask1_dev || !prob->dpts0_dev || !prob->homo_dev || !prob->feat0s_dev ||
                          !prob->feat1_dev || !prob->grad1_dev || !prob->weights_dev || prob->N < 1))
    return SAGE_E_INVALID;
  if (prob->use_keypoints &&
      (!prob->kp_dpts0_dev || !prob->kp_homo0_dev || prob->NK < 1 ||
       (dof == 6 ? !prob->kp_matched_2d_dev : (!prob->kp_matched_dpts1_dev || !prob->kp_matched_homo1_dev))))
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

