// operators.hip -- workspaces and the per-edge operator API behind the C ABI: the drop-in replacements of the reference's
// df::*_calculate free functions (photometric_factor_kernels.h:9-70, geometric_factor_kernels.h:18-48, reprojection /
// match-geometry kernels) and the keyframe input producers.
#include "runtime_internal.h"

extern "C" int sage_workspace_create(void *hip_stream, SageWorkspace **out)
{
  if (!out)
    return SAGE_E_INVALID;
  int ndev = 0;
  SAGE_HIP(hipGetDeviceCount(&ndev));
  if (ndev < 1)
    return (int)hipErrorNoDevice;
  SageWorkspace *ws = new SageWorkspace();
  ws->stream = reinterpret_cast<hipStream_t>(hip_stream);
  const int rc = ws->host_stats.reserve(sizeof(WsHostStats));
  if (rc)
  {
    delete ws;
    return rc;
  }
  std::memset(ws->hs(), 0, sizeof(WsHostStats));
  *out = ws;
  return SAGE_OK;
}

extern "C" void sage_workspace_destroy(SageWorkspace *ws) { delete ws; } // (its buffers go with it: DevBuf, PinnedBuf)

// the work list of ONE edge of N samples in the workspace's buffers, bound into lc with room for `partial_floats` per work
// item.  Built and uploaded when the workspace holds another list (kind, N); N == 0 is one empty workgroup, so that the
// finalize sees zeros
static int ws_bind_work(SageWorkspace *ws, WorkKind kind, int N, size_t partial_floats, LaunchCommon *lc)
{
  if (!ws || (N < 0 && kind == WorkKind::dense)) // (the tracker's entry points have never refused N < 0: the list of N == 0)
    return SAGE_E_INVALID;
  int rc;
  if (ws->list_kind != kind || ws->list_N != N)
  {
    WorkList wl;
    wl.build(std::vector<int>{N}, kind == WorkKind::tracker ? 1 : 0);
    if (wl.work.empty())
      wl.work.push_back(WorkItem{0, 0});
    if (wl.edge_tiles[0] == 0)
      wl.edge_tiles[0] = 1;
    ws->list_kind = WorkKind::none; // (until all three arrays are the new list's)
    if ((rc = upload(ws->work, wl.work, ws->stream)) || (rc = upload(ws->edge_first, wl.edge_first, ws->stream)) ||
        (rc = upload(ws->edge_tiles, wl.edge_tiles, ws->stream)))
      return rc;
    SAGE_HIP(hipStreamSynchronize(ws->stream)); // wl goes out of scope
    ws->list_kind = kind;
    ws->list_N = N;
    ws->n_work = (int)wl.work.size();
    ws->tiles_per_block = wl.tiles_per_block;
  }
  if ((rc = ws->partials.reserve((size_t)ws->n_work * partial_floats * sizeof(float))))
    return rc;
  lc->work = ws->work.as<WorkItem>();
  lc->edge_first = ws->edge_first.as<int32_t>();
  lc->edge_tiles = ws->edge_tiles.as<int32_t>();
  lc->n_work = ws->n_work;
  lc->n_edges = 1;
  lc->partials = ws->partials.as<float>();
  lc->tiles_per_block = ws->tiles_per_block;
  return SAGE_OK;
}

__global__ void ticket_kernel(volatile unsigned *ticket, unsigned epoch)
{
  __threadfence_system();
  *ticket = epoch;
}

unsigned ws_ticket_next(SageWorkspace *ws)
{
  if (++ws->ticket_epoch == 0)
    ws->ticket_epoch = 1;
  return ws->ticket_epoch;
}

int ws_ticket_await(SageWorkspace *ws, unsigned epoch)
{
  volatile unsigned *ticket = &ws->hs()->ticket;
  if (!spin_until([=] { return *ticket == epoch; }))
    SAGE_HIP(hipStreamSynchronize(ws->stream)); // (a long queue ahead of this operator: wait the ordinary way)
  return SAGE_OK;
}

int ws_ticket_wait(SageWorkspace *ws)
{
  const unsigned epoch = ws_ticket_next(ws);
  hipLaunchKernelGGL(ticket_kernel, dim3(1), dim3(1), 0, ws->stream, &ws->hs()->ticket, epoch);
  SAGE_HIP(hipGetLastError());
  return ws_ticket_await(ws, epoch);
}

// the public entry points' half of an operator: its kernels have been enqueued (rc) with the workspace's own stats slot as
// their destination; wait for them and hand {error, inliers} to the caller
static float *ws_own_stats(SageWorkspace *ws) { return ws ? ws->hs()->stats : nullptr; }
static int ws_fetch_stats(int rc, SageWorkspace *ws, float *error_host, float *num_inliers_host)
{
  if (rc || (rc = ws_ticket_wait(ws)))
    return rc;
  if (error_host)
    *error_host = ws->hs()->stats[0];
  if (num_inliers_host)
    *num_inliers_host = ws->hs()->stats[1];
  return SAGE_OK;
}

// source depths of a per-edge operator call: the kernels read them from a map indexed by loc1d.  With few samples only
// those pixels are formed (N*CS reads instead of H*W*CS); the photometric kernels also range-check loc1d against H*W
// (PhotoEdge::HW), so a bad location reads nothing -- the reference's tensor index() would throw on it.
static int operator_depths(SageWorkspace *ws, int CS, const float *bias0, const float *basis0, const float *code0,
                           float scale0, const void *loc, int loc_is_i64, int N, int H, int W)
{
  int rc;
  if ((rc = ws->dpt0.reserve((size_t)H * W * sizeof(float))))
    return rc;
  if ((long long)N * 2 <= (long long)H * W)
    SAGE_HIP(launch_depth_samples(ws->stream, CS, ws->dpt0.as<float>(), bias0, basis0, code0, scale0, loc, loc_is_i64,
                                  N, H * W));
  else
    SAGE_HIP(launch_depth_and_grad(ws->stream, CS, ws->dpt0.as<float>(), nullptr, bias0, basis0, code0, nullptr,
                                   scale0, H, W));
  return SAGE_OK;
}


// =====================================================================================================
// per-edge operator API
// =====================================================================================================
// Every operator family is an enqueue function -- validate, reserve, launch; its kernels write {error, inliers} to `stats`
// and nobody waits -- and the public entry points: the enqueue with the workspace's own stats slot, then ws_fetch_stats.
// The jac and the error variant of a family share the enqueue; where their rules differ (which pointers may be NULL) it
// says so.
static int photo_enqueue(SageWorkspace *ws, bool jac, float *AtA, float *Atb, float *stats, const float *R10,
                         const float *t10, const float *R0, const float *t0, const float *R1, const float *t1,
                         const float *bias0, const float *basis0, const float *code0, const float *mask1,
                         const int64_t *loc1d, const float *homo, const float *feat0, const float *feat1,
                         const float *grad1, float scale0, const SagePyramid *pyr, float eps, const float *weights_host,
                         int N, int FS, int CS)
{
  if (!ws || !pyr || !weights_host || !bias0 || !basis0 || !code0 || !mask1 || !loc1d || !homo || !feat0 || !feat1)
    return SAGE_E_INVALID;
  // jac: the absolute poses, R10 / t10 optional (the kernel forms them); error: the relative pose only
  if (jac ? (!AtA || !Atb || !R0 || !t0 || !R1 || !t1 || !grad1) : (!R10 || !t10))
    return SAGE_E_INVALID;
  if (!supported(CS, FS) || pyr->levels < 1 || pyr->levels > SAGE_MAX_LEVELS)
    return SAGE_E_UNSUPPORTED;
  LaunchCommon lc;
  int rc = ws_bind_work(ws, WorkKind::dense, N, jac ? photo_partial_floats(CS) : 2, &lc);
  if (rc)
    return rc;
  // depth map of the source keyframe at (code0, scale0): the kernel reads its sample depths from it
  if ((rc = operator_depths(ws, CS, bias0, basis0, code0, scale0, loc1d, 1, N, (int)pyr->cam[0].h, (int)pyr->cam[0].w)))
    return rc;
  PhotoEdge e{};
  e.dpt0 = ws->dpt0.as<float>();
  e.feat0 = feat0; e.feat1 = feat1; e.grad1 = grad1; e.bias0 = bias0; e.basis0 = basis0; e.mask1 = mask1;
  e.homo = homo; e.loc = loc1d; e.loc_is_i64 = 1;
  e.R0 = R0; e.t0 = t0; e.R1 = R1; e.t1 = t1; e.R10 = R10; e.t10 = R10 ? t10 : nullptr;
  e.code0 = code0; e.scale0 = nullptr; e.scale0_val = scale0; e.N = N;
  if (jac)
    SAGE_HIP(launch_photo_linearize(ws->stream, CS, FS, &e, nullptr, lc, *pyr, weights_host, eps, EdgeOut{AtA, Atb, stats}));
  else
    SAGE_HIP(launch_photo_error(ws->stream, CS, FS, &e, nullptr, lc, *pyr, weights_host, eps, stats));
  return SAGE_OK;
}

extern "C" int sage_photometric_jac_error_calculate(
    SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host, float *num_inliers_host,
    const float *R10, const float *t10, const float *R0, const float *t0, const float *R1, const float *t1,
    const float *bias0, const float *basis0, const float *code0, const float *mask1, const int64_t *loc1d,
    const float *homo, const float *feat0, const float *feat1, const float *grad1, float scale0,
    const SagePyramid *pyr, float eps, const float *weights_host, int N, int FS, int CS)
{
  return ws_fetch_stats(photo_enqueue(ws, true, AtA_dev, Atb_dev, ws_own_stats(ws), R10, t10, R0, t0, R1, t1, bias0, basis0,
                                      code0, mask1, loc1d, homo, feat0, feat1, grad1, scale0, pyr, eps, weights_host, N, FS,
                                      CS),
                        ws, error_host, num_inliers_host);
}

extern "C" int sage_photometric_error_calculate(
    SageWorkspace *ws, float *error_host, float *num_inliers_host, const float *R10, const float *t10,
    const float *bias0, const float *basis0, const float *code0, const float *mask1, const int64_t *loc1d,
    const float *homo, const float *feat0, const float *feat1, float scale0, const SagePyramid *pyr, float eps,
    const float *weights_host, int N, int FS, int CS)
{
  return ws_fetch_stats(photo_enqueue(ws, false, nullptr, nullptr, ws_own_stats(ws), R10, t10, nullptr, nullptr, nullptr,
                                      nullptr, bias0, basis0, code0, mask1, loc1d, homo, feat0, feat1, nullptr, scale0, pyr,
                                      eps, weights_host, N, FS, CS),
                        ws, error_host, num_inliers_host);
}

int track_photo_enqueue(SageWorkspace *ws, bool jac, int dof, float *AtA, float *Atb, float *stats, const float *R,
                        const float *t, const float *mask1, const float *dpts0, const float *homo, const float *feat0s,
                        const float *feat1, const float *grad1, const SagePyramid *pyr, float scale0, float eps,
                        const float *weights_dev, int N, int FS)
{
  if (!ws || !pyr || !R || !t || !mask1 || !dpts0 || !homo || !feat0s || !feat1 || !weights_dev ||
      (jac && (!grad1 || !AtA || !Atb)))
    return SAGE_E_INVALID;
  if ((FS != 16 && FS != 32) || pyr->levels < 1 || pyr->levels > SAGE_MAX_LEVELS)
    return SAGE_E_UNSUPPORTED;
  LaunchCommon lc{};
  const int rc = ws_bind_work(ws, WorkKind::tracker, N, kTrackScalars, &lc);
  if (rc)
    return rc;
  TrackEdge e{};
  e.feat0s = feat0s; e.feat1 = feat1; e.grad1 = grad1; e.mask1 = mask1; e.homo = homo; e.dpts0 = dpts0;
  e.R = R; e.t = t; e.weights = weights_dev; e.scale0 = scale0; e.N = N;
  if (jac)
    SAGE_HIP(launch_track_linearize(ws->stream, dof, FS, e, lc, *pyr, eps, EdgeOut{AtA, Atb, stats}));
  else
    SAGE_HIP(launch_track_error(ws->stream, FS, e, lc, *pyr, eps, stats));
  return SAGE_OK;
}

extern "C" int sage_tracker_photo_jac_error_calculate(
    SageWorkspace *ws, int dof, float *AtA_dev, float *Atb_dev, float *error_host, float *num_inliers_host,
    const float *R, const float *t, const float *mask1, const float *dpts0, const float *homo,
    const float *feat0s, const float *feat1, const float *grad1, const SagePyramid *pyr, float scale0, float eps,
    const float *weights_dev, int N, int FS)
{
  if (dof != 6 && dof != 7)
    return SAGE_E_INVALID;
  return ws_fetch_stats(track_photo_enqueue(ws, true, dof, AtA_dev, Atb_dev, ws_own_stats(ws), R, t, mask1, dpts0, homo,
                                            feat0s, feat1, grad1, pyr, scale0, eps, weights_dev, N, FS),
                        ws, error_host, num_inliers_host);
}

extern "C" int sage_tracker_photo_error_calculate(
    SageWorkspace *ws, float *error_host, float *num_inliers_host, const float *R, const float *t,
    const float *mask1, const float *dpts0, const float *homo, const float *feat0s, const float *feat1,
    const SagePyramid *pyr, float eps, const float *weights_dev, int N, int FS)
{
  return ws_fetch_stats(track_photo_enqueue(ws, false, 6, nullptr, nullptr, ws_own_stats(ws), R, t, mask1, dpts0, homo,
                                            feat0s, feat1, nullptr, pyr, 1.0f, eps, weights_dev, N, FS),
                        ws, error_host, num_inliers_host);
}

static int geo_enqueue(SageWorkspace *ws, bool jac, float *AtA, float *Atb, float *stats, const float *R10,
                       const float *t10, const float *R0, const float *t0, const float *R1, const float *t1,
                       const float *bias0, const float *basis0, const float *code0, const float *dpt1,
                       const float *dgrad1, const float *basis1, const float *mask1, const int32_t *loc1d,
                       const float *homo, float scale0, float scale1, const SageCamera *cam, float eps, float loss_param,
                       float weight, int N, int CS)
{
  if (!ws || !cam || !bias0 || !basis0 || !code0 || !dpt1 || !mask1 || !loc1d || !homo)
    return SAGE_E_INVALID;
  // jac: the absolute poses, R10 / t10 optional (the kernel forms them); error: the relative pose only
  if (jac ? (!AtA || !Atb || !R0 || !t0 || !R1 || !t1 || !dgrad1 || !basis1) : (!R10 || !t10))
    return SAGE_E_INVALID;
  if (CS != 16 && CS != 32)
    return SAGE_E_UNSUPPORTED;
  LaunchCommon lc;
  int rc = ws_bind_work(ws, WorkKind::dense, N, jac ? geo_partial_floats(CS) : 2, &lc);
  if (rc)
    return rc;
  // depth map of the source keyframe at (code0, scale0): the kernel reads its sample depths from it
  if ((rc = operator_depths(ws, CS, bias0, basis0, code0, scale0, loc1d, 0, N, (int)cam->h, (int)cam->w)))
    return rc;
  GeoEdge e{};
  e.dpt0 = ws->dpt0.as<float>();
  e.bias0 = bias0; e.basis0 = basis0; e.dpt1 = dpt1; e.dgrad1 = dgrad1; e.basis1 = basis1; e.mask1 = mask1;
  e.homo = homo; e.loc = loc1d; e.loc_is_i64 = 0;
  e.R0 = R0; e.t0 = t0; e.R1 = R1; e.t1 = t1; e.R10 = R10; e.t10 = R10 ? t10 : nullptr;
  e.code0 = code0; e.scale0 = nullptr; e.scale1 = nullptr; e.scale0_val = scale0; e.scale1_val = scale1; e.N = N;
  if (jac)
    SAGE_HIP(launch_geo_linearize(ws->stream, CS, &e, nullptr, lc, *cam, eps, loss_param, weight, EdgeOut{AtA, Atb, stats}));
  else
    SAGE_HIP(launch_geo_error(ws->stream, CS, &e, nullptr, lc, *cam, eps, loss_param, weight, stats));
  return SAGE_OK;
}

extern "C" int sage_geometric_jac_error_calculate(
    SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host, float *num_inliers_host,
    const float *R10, const float *t10, const float *R0, const float *t0, const float *R1, const float *t1,
    const float *bias0, const float *basis0, const float *code0, const float *dpt1, const float *dgrad1,
    const float *basis1, const float *mask1, const int32_t *loc1d, const float *homo, float scale0, float scale1,
    const SageCamera *cam, float eps, float loss_param, float weight, int N, int CS)
{
  return ws_fetch_stats(geo_enqueue(ws, true, AtA_dev, Atb_dev, ws_own_stats(ws), R10, t10, R0, t0, R1, t1, bias0, basis0,
                                    code0, dpt1, dgrad1, basis1, mask1, loc1d, homo, scale0, scale1, cam, eps, loss_param,
                                    weight, N, CS),
                        ws, error_host, num_inliers_host);
}

extern "C" int sage_geometric_error_calculate(
    SageWorkspace *ws, float *error_host, float *num_inliers_host, const float *R10, const float *t10,
    const float *bias0, const float *basis0, const float *code0, const float *dpt1, const float *mask1,
    const int32_t *loc1d, const float *homo, float scale0, const SageCamera *cam, float eps, float loss_param,
    float weight, int N, int CS)
{
  return ws_fetch_stats(geo_enqueue(ws, false, nullptr, nullptr, ws_own_stats(ws), R10, t10, nullptr, nullptr, nullptr,
                                    nullptr, bias0, basis0, code0, dpt1, nullptr, nullptr, mask1, loc1d, homo, scale0, 1.f,
                                    cam, eps, loss_param, weight, N, CS),
                        ws, error_host, num_inliers_host);
}

extern "C" int sage_depth_and_grad(SageWorkspace *ws, float *dpt, float *grad, const float *bias, const float *basis,
                                   const float *code, float scale, int H, int W, int CS)
{
  if (!ws || !dpt || !bias || !basis || !code)
    return SAGE_E_INVALID;
  if (CS != 16 && CS != 32)
    return SAGE_E_UNSUPPORTED;
  SAGE_HIP(launch_depth_and_grad(ws->stream, CS, dpt, grad, bias, basis, code, nullptr, scale, H, W));
  return SAGE_OK;
}

// ---- sparse reprojection factor (keypoint_kernels.hip) ----
static int reproj_enqueue(SageWorkspace *ws, bool tracker, bool jac, float *AtA, float *Atb, float *stats, ReprojParams p,
                          const SageCamera *cam, int CS)
{
  const int N = p.N;
  if (!ws || !cam || N < 0 || !p.R10 || !p.t10 || (N > 0 && (!p.homo || !p.matched)) || (jac && (!AtA || !Atb)))
    return SAGE_E_INVALID;
  if (!tracker && (!p.bias0 || !p.basis0 || !p.code0 || (N > 0 && !p.loc) || (jac && (!p.R0 || !p.t0 || !p.R1 || !p.t1))))
    return SAGE_E_INVALID;
  if (tracker && N > 0 && !p.dpts0)
    return SAGE_E_INVALID;
  if (!tracker && CS != 16 && CS != 32)
    return SAGE_E_UNSUPPORTED;
  p.cam = *cam;
  int rc;
  if ((rc = ws->misc.reserve(kp_scratch_floats(kReprojRows, N, reproj_dim(tracker ? 1 : 0, CS)) * sizeof(float))))
    return rc;
  SAGE_HIP(launch_reproj(ws->stream, CS, tracker, jac, p, ws->misc.as<float>(), KpOut{AtA, Atb, stats}));
  return SAGE_OK;
}

extern "C" int sage_reprojection_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host,
                                                     float *num_inliers_host, const float *R10, const float *t10,
                                                     const float *R0, const float *t0, const float *R1, const float *t1,
                                                     const float *bias0, const float *basis0, const float *code0,
                                                     const int32_t *loc1d, const float *homo, const float *matched_2d,
                                                     float scale0, const SageCamera *cam, float eps, float loss_param,
                                                     float weight, int N, int CS)
{
  ReprojParams p{};
  p.R10 = R10; p.t10 = t10; p.R0 = R0; p.t0 = t0; p.R1 = R1; p.t1 = t1;
  p.bias0 = bias0; p.basis0 = basis0; p.code0 = code0; p.loc = loc1d; p.homo = homo; p.matched = matched_2d;
  p.scale0 = scale0; p.eps = eps; p.loss_param = loss_param; p.weight = weight; p.N = N;
  return ws_fetch_stats(reproj_enqueue(ws, false, true, AtA_dev, Atb_dev, ws_own_stats(ws), p, cam, CS), ws, error_host,
                        num_inliers_host);
}

extern "C" int sage_reprojection_error_calculate(SageWorkspace *ws, float *error_host, float *num_inliers_host,
                                                 const float *R10, const float *t10, const float *bias0,
                                                 const float *basis0, const float *code0, const int32_t *loc1d,
                                                 const float *homo, const float *matched_2d, float scale0,
                                                 const SageCamera *cam, float eps, float loss_param, float weight, int N,
                                                 int CS)
{
  ReprojParams p{};
  p.R10 = R10; p.t10 = t10;
  p.bias0 = bias0; p.basis0 = basis0; p.code0 = code0; p.loc = loc1d; p.homo = homo; p.matched = matched_2d;
  p.scale0 = scale0; p.eps = eps; p.loss_param = loss_param; p.weight = weight; p.N = N;
  return ws_fetch_stats(reproj_enqueue(ws, false, false, nullptr, nullptr, ws_own_stats(ws), p, cam, CS), ws, error_host,
                        num_inliers_host);
}

int track_reproj_enqueue(SageWorkspace *ws, bool jac, float *AtA, float *Atb, float *stats, const float *R, const float *t,
                         const float *sampled_dpts0, const float *homo, const float *matched_2d, const SageCamera *cam,
                         float eps, float loss_param, float weight, int N)
{
  ReprojParams p{}; // tracker: R10 / t10 = the relative pose, depths handed over
  p.R10 = R; p.t10 = t; p.dpts0 = sampled_dpts0; p.homo = homo; p.matched = matched_2d;
  p.scale0 = 1.f; p.eps = eps; p.loss_param = loss_param; p.weight = weight; p.N = N;
  return reproj_enqueue(ws, true, jac, AtA, Atb, stats, p, cam, 16);
}

extern "C" int sage_tracker_reproj_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev,
                                                       float *error_host, float *num_inliers_host, const float *R,
                                                       const float *t, const float *sampled_dpts0, const float *homo,
                                                       const float *matched_2d, const SageCamera *cam, float eps,
                                                       float loss_param, float weight, int N)
{
  return ws_fetch_stats(track_reproj_enqueue(ws, true, AtA_dev, Atb_dev, ws_own_stats(ws), R, t, sampled_dpts0, homo,
                                             matched_2d, cam, eps, loss_param, weight, N),
                        ws, error_host, num_inliers_host);
}

extern "C" int sage_tracker_reproj_error_calculate(SageWorkspace *ws, float *error_host, float *num_inliers_host,
                                                   const float *R, const float *t, const float *sampled_dpts0,
                                                   const float *homo, const float *matched_2d, const SageCamera *cam,
                                                   float eps, float loss_param, float weight, int N)
{
  return ws_fetch_stats(track_reproj_enqueue(ws, false, nullptr, nullptr, ws_own_stats(ws), R, t, sampled_dpts0, homo,
                                             matched_2d, cam, eps, loss_param, weight, N),
                        ws, error_host, num_inliers_host);
}

// ---- match-geometry factors (keypoint_kernels.hip) ----
static int mg_enqueue(SageWorkspace *ws, int mode, bool jac, float *AtA, float *Atb, float *stats, const MgParams &p, int CS)
{
  if (!ws || p.N < 1 || !p.R10 || !p.t10 || !p.homo0 || !p.homo1 || (jac && (!AtA || !Atb)))
    return SAGE_E_INVALID;
  if (mode == 0 && (!p.bias0 || !p.bias1 || !p.basis0 || !p.basis1 || !p.code0 || !p.code1 || !p.loc0 || !p.loc1))
    return SAGE_E_INVALID;
  if (mode != 0 && (!p.dpts0 || !p.dpts1))
    return SAGE_E_INVALID;
  if (mode <= 1 && jac && (!p.R0 || !p.t0 || !p.R1 || !p.t1))
    return SAGE_E_INVALID;
  if (p.loss < 0 || p.loss > 3 || (p.loss == SAGE_LOSS_UNBIASED && mode != 0) || (mode != 0 && p.loss != SAGE_LOSS_FAIR))
    return SAGE_E_INVALID;
  if (mode == 0 && CS != 16 && CS != 32)
    return SAGE_E_UNSUPPORTED;
  int rc;
  if ((rc = ws->misc.reserve(kp_scratch_floats(kMgRows, p.N, mg_dim(mode, CS)) * sizeof(float))))
    return rc;
  SAGE_HIP(launch_match_geom(ws->stream, mode, CS, jac, p, ws->misc.as<float>(), KpOut{AtA, Atb, stats}));
  return SAGE_OK;
}

extern "C" int sage_match_geometry_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev,
                                                       float *error_host, const float *R10, const float *t10,
                                                       const float *R0, const float *t0, const float *R1,
                                                       const float *t1, const float *bias0, const float *bias1,
                                                       const float *basis0, const float *basis1, const float *code0,
                                                       const float *code1, const float *homo0,
                                                       const float *matched_homo1, const int32_t *loc1d_0,
                                                       const int32_t *matched_loc1d_1, float scale0, float scale1,
                                                       float loss_param, float weight, int loss, int N, int CS)
{
  MgParams p{};
  p.R10 = R10; p.t10 = t10; p.homo0 = homo0; p.homo1 = matched_homo1;
  p.scale0 = scale0; p.scale1 = scale1; p.loss_param = loss_param; p.weight = weight; p.loss = loss; p.N = N;
  p.R0 = R0; p.t0 = t0; p.R1 = R1; p.t1 = t1;
  p.bias0 = bias0; p.bias1 = bias1; p.basis0 = basis0; p.basis1 = basis1; p.code0 = code0; p.code1 = code1;
  p.loc0 = loc1d_0; p.loc1 = matched_loc1d_1;
  return ws_fetch_stats(mg_enqueue(ws, 0, true, AtA_dev, Atb_dev, ws_own_stats(ws), p, CS), ws, error_host, nullptr);
}

extern "C" int sage_match_geometry_error_calculate(SageWorkspace *ws, float *error_host, const float *R10,
                                                   const float *t10, const float *bias0, const float *bias1,
                                                   const float *basis0, const float *basis1, const float *code0,
                                                   const float *code1, const float *homo0, const float *matched_homo1,
                                                   const int32_t *loc1d_0, const int32_t *matched_loc1d_1, float scale0,
                                                   float scale1, float loss_param, float weight, int loss, int N, int CS)
{
  MgParams p{};
  p.R10 = R10; p.t10 = t10; p.homo0 = homo0; p.homo1 = matched_homo1;
  p.scale0 = scale0; p.scale1 = scale1; p.loss_param = loss_param; p.weight = weight; p.loss = loss; p.N = N;
  p.bias0 = bias0; p.bias1 = bias1; p.basis0 = basis0; p.basis1 = basis1; p.code0 = code0; p.code1 = code1;
  p.loc0 = loc1d_0; p.loc1 = matched_loc1d_1;
  return ws_fetch_stats(mg_enqueue(ws, 0, false, nullptr, nullptr, ws_own_stats(ws), p, CS), ws, error_host, nullptr);
}

extern "C" int sage_loop_mg_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev, float *error_host,
                                                const float *R10, const float *t10, const float *R0, const float *t0,
                                                const float *R1, const float *t1, const float *unscaled_dpts0,
                                                const float *matched_unscaled_dpts1, const float *homo0,
                                                const float *matched_homo1, float scale0, float scale1, float loss_param,
                                                float weight, int N)
{
  MgParams p{};
  p.R10 = R10; p.t10 = t10; p.homo0 = homo0; p.homo1 = matched_homo1;
  p.scale0 = scale0; p.scale1 = scale1; p.loss_param = loss_param; p.weight = weight; p.loss = SAGE_LOSS_FAIR; p.N = N;
  p.R0 = R0; p.t0 = t0; p.R1 = R1; p.t1 = t1; p.dpts0 = unscaled_dpts0; p.dpts1 = matched_unscaled_dpts1;
  return ws_fetch_stats(mg_enqueue(ws, 1, true, AtA_dev, Atb_dev, ws_own_stats(ws), p, 16), ws, error_host, nullptr);
}

extern "C" int sage_loop_mg_error_calculate(SageWorkspace *ws, float *error_host, const float *R10, const float *t10,
                                            const float *unscaled_dpts0, const float *matched_unscaled_dpts1,
                                            const float *homo0, const float *matched_homo1, float scale0, float scale1,
                                            float loss_param, float weight, int N)
{
  MgParams p{};
  p.R10 = R10; p.t10 = t10; p.homo0 = homo0; p.homo1 = matched_homo1;
  p.scale0 = scale0; p.scale1 = scale1; p.loss_param = loss_param; p.weight = weight; p.loss = SAGE_LOSS_FAIR; p.N = N;
  p.dpts0 = unscaled_dpts0; p.dpts1 = matched_unscaled_dpts1;
  return ws_fetch_stats(mg_enqueue(ws, 1, false, nullptr, nullptr, ws_own_stats(ws), p, 16), ws, error_host, nullptr);
}

// tracker: R10 / t10 = the relative pose, depths handed over; mode 2 = pose only, 3 = pose and scale
int track_match_geom_enqueue(SageWorkspace *ws, int mode, bool jac, float *AtA, float *Atb, float *stats, const float *R,
                             const float *t, const float *sampled_dpts0, const float *matched_dpts1, const float *homo0,
                             const float *matched_homo1, float scale0, float loss_param, float weight, int N)
{
  MgParams p{};
  p.R10 = R; p.t10 = t; p.homo0 = homo0; p.homo1 = matched_homo1;
  p.scale0 = scale0; p.scale1 = 1.f; p.loss_param = loss_param; p.weight = weight; p.loss = SAGE_LOSS_FAIR; p.N = N;
  p.dpts0 = sampled_dpts0; p.dpts1 = matched_dpts1;
  return mg_enqueue(ws, mode, jac, AtA, Atb, stats, p, 16);
}

extern "C" int sage_tracker_match_geom_jac_error_calculate(SageWorkspace *ws, float *AtA_dev, float *Atb_dev,
                                                           float *error_host, const float *R, const float *t,
                                                           const float *sampled_dpts0, const float *matched_dpts1,
                                                           const float *homo0, const float *matched_homo1, float scale0,
                                                           float loss_param, float weight, int with_scale, int N)
{
  return ws_fetch_stats(track_match_geom_enqueue(ws, with_scale ? 3 : 2, true, AtA_dev, Atb_dev, ws_own_stats(ws), R, t,
                                                 sampled_dpts0, matched_dpts1, homo0, matched_homo1, scale0, loss_param,
                                                 weight, N),
                        ws, error_host, nullptr);
}

extern "C" int sage_tracker_match_geom_error_calculate(SageWorkspace *ws, float *error_host, const float *R,
                                                       const float *t, const float *sampled_dpts0,
                                                       const float *matched_dpts1, const float *homo0,
                                                       const float *matched_homo1, float loss_param, float weight, int N)
{
  return ws_fetch_stats(track_match_geom_enqueue(ws, 2, false, nullptr, nullptr, ws_own_stats(ws), R, t, sampled_dpts0,
                                                 matched_dpts1, homo0, matched_homo1, 1.f, loss_param, weight, N),
                        ws, error_host, nullptr);
}

extern "C" int sage_cycle_match(SageWorkspace *ws, const float *desc0, const float *desc1, const int64_t *kp_loc1d_0,
                                int K, int C, int H, int W, float cyc_thresh, int64_t *raw_matched_loc1d_1,
                                int64_t *cyc_matched_loc1d_0, int32_t *inlier_flags, int *n_inliers_host)
{
  if (!ws || K < 0 || C < 1 || C > 1024 || H < 1 || W < 1 || !n_inliers_host ||
      (K > 0 && (!desc0 || !desc1 || !kp_loc1d_0 || !raw_matched_loc1d_1 || !cyc_matched_loc1d_0 || !inlier_flags)))
    return SAGE_E_INVALID;
  int rc = ws->misc.reserve(sizeof(int));
  if (rc)
    return rc;
  SAGE_HIP(hipMemsetAsync(ws->misc.p, 0, sizeof(int), ws->stream));
  SAGE_HIP(launch_cycle_match(ws->stream, desc0, desc1, reinterpret_cast<const long long *>(kp_loc1d_0), K, C, H, W,
                              cyc_thresh, reinterpret_cast<long long *>(raw_matched_loc1d_1),
                              reinterpret_cast<long long *>(cyc_matched_loc1d_0), inlier_flags, ws->misc.as<int>()));
  SAGE_HIP(hipMemcpyAsync(n_inliers_host, ws->misc.p, sizeof(int), hipMemcpyDeviceToHost, ws->stream));
  SAGE_HIP(hipStreamSynchronize(ws->stream));
  return SAGE_OK;
}

extern "C" int sage_valid_locations(SageWorkspace *ws, const float *mask_dev, const SageCamera *cam,
                                    int64_t *loc1d_dev, float *homo_dev, int *n_valid_host)
{
  if (!ws || !mask_dev || !cam || !loc1d_dev || !homo_dev || !n_valid_host)
    return SAGE_E_INVALID;
  int rc = ws->misc.reserve(sizeof(int));
  if (rc)
    return rc;
  SAGE_HIP(launch_valid_locations(ws->stream, mask_dev, *cam, reinterpret_cast<long long *>(loc1d_dev), homo_dev,
                                  ws->misc.as<int>()));
  SAGE_HIP(hipMemcpyAsync(n_valid_host, ws->misc.p, sizeof(int), hipMemcpyDeviceToHost, ws->stream));
  SAGE_HIP(hipStreamSynchronize(ws->stream));
  return SAGE_OK;
}

extern "C" int sage_sample_locations(SageWorkspace *ws, const int64_t *valid_loc1d_dev, const float *valid_homo_dev,
                                     int n_valid, int64_t seed, int num_samples, int64_t *loc1d_dev, float *homo_dev,
                                     int *n_out_host)
{
  if (!ws || !valid_loc1d_dev || !valid_homo_dev || n_valid < 0 || num_samples < 0 || !loc1d_dev || !homo_dev ||
      !n_out_host)
    return SAGE_E_INVALID;
  std::vector<int64_t> idx((size_t)std::max(n_valid, 1));
  int rc = sage_shuffle_indices(seed, n_valid, idx.data());
  if (rc)
    return rc;
  const int n = std::min(num_samples, n_valid); // mapper.cpp:1336
  if ((rc = ws->misc.reserve((size_t)std::max(n, 1) * sizeof(int64_t))))
    return rc;
  if (n > 0)
  {
    SAGE_HIP(hipMemcpyAsync(ws->misc.p, idx.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ws->stream));
    SAGE_HIP(launch_gather_locations(ws->stream, reinterpret_cast<const long long *>(valid_loc1d_dev), valid_homo_dev,
                                     ws->misc.as<long long>(), n, reinterpret_cast<long long *>(loc1d_dev), homo_dev));
    SAGE_HIP(hipStreamSynchronize(ws->stream)); // idx goes out of scope
  }
  *n_out_host = n;
  return SAGE_OK;
}

extern "C" int sage_sort_locations(SageWorkspace *ws, const int64_t *loc1d_dev, const float *homo_dev, int n, int H,
                                   int W, int64_t *loc1d_out_dev, float *homo_out_dev, int *sorted_host)
{
  // (an empty list has no arrays: n = 0 is answered "sorted" whatever the pointers are)
  if (!ws || n < 0 || H < 1 || W < 1 || !sorted_host ||
      (n > 0 && (!loc1d_dev || !homo_dev || !loc1d_out_dev || !homo_out_dev || loc1d_out_dev == loc1d_dev ||
                 homo_out_dev == homo_dev)))
    return SAGE_E_INVALID;
  if (n == 0)
  {
    *sorted_host = 1;
    return SAGE_OK;
  }
  const int HW = H * W;
  // scratch: [item | status (2 ints) | mark plane]
  const size_t off_status = (sizeof(SortItem) + 15) / 16 * 16, off_mark = off_status + 16;
  int rc = ws->misc.reserve(off_mark + (size_t)HW * sizeof(int));
  if (rc)
    return rc;
  char *base = ws->misc.as<char>();
  const SortItem it{reinterpret_cast<const long long *>(loc1d_dev), homo_dev, reinterpret_cast<long long *>(loc1d_out_dev),
                    homo_out_dev, n};
  int status[2] = {0, 0};
  SAGE_HIP(hipMemcpyAsync(base, &it, sizeof(it), hipMemcpyHostToDevice, ws->stream));
  SAGE_HIP(launch_sort_locations(ws->stream, reinterpret_cast<const SortItem *>(base), 1, n, HW,
                                 reinterpret_cast<int *>(base + off_mark), reinterpret_cast<int *>(base + off_status)));
  SAGE_HIP(hipMemcpyAsync(status, base + off_status, sizeof(status), hipMemcpyDeviceToHost, ws->stream));
  SAGE_HIP(hipStreamSynchronize(ws->stream)); // `it` and `status` are locals
  if (status[0] > 0)
    return SAGE_E_INVALID;
  *sorted_host = status[1] == n;
  if (!*sorted_host && n > 0)
  {
    // a pixel listed twice: keep the caller's order (and every sample)
    SAGE_HIP(hipMemcpyAsync(loc1d_out_dev, loc1d_dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, ws->stream));
    SAGE_HIP(hipMemcpyAsync(homo_out_dev, homo_dev, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, ws->stream));
    SAGE_HIP(hipStreamSynchronize(ws->stream));
  }
  return SAGE_OK;
}

extern "C" int sage_gaussian_pyramid_with_grad(SageWorkspace *ws, float *pyr_dev, float *grad_dev,
                                               const float *feat, const float *mask, const SagePyramid *pyr, int FS)
{
  if (!ws || !pyr_dev || !grad_dev || !feat || !mask || !pyr)
    return SAGE_E_INVALID;
  const int H = (int)pyr->cam[0].h, W = (int)pyr->cam[0].w;
  for (int l = 0; l + 1 < pyr->levels; ++l) // the reference's conv / camera / mask pyramids only agree for even sizes
    if (((int)pyr->cam[l].h & 1) || ((int)pyr->cam[l].w & 1))
      return SAGE_E_UNSUPPORTED;
  const size_t scratch = ((size_t)FS * (H / 2) * (W / 2) + (size_t)(H / 2) * (W / 2)) * 2 * sizeof(float);
  int rc = ws->misc.reserve(scratch);
  if (rc)
    return rc;
  SAGE_HIP(launch_gaussian_pyramid_with_grad(ws->stream, pyr_dev, grad_dev, feat, mask, *pyr, FS,
                                             ws->misc.as<float>()));
  return SAGE_OK;
}

