// window_tsdf.hip -- from a window to a fused surface: the window's keyframes into a TSDF volume in one pass
// (sage_window_fuse_tsdf: depth maps at the current variables, the window's poses, camera and video mask, the sigma maps of the
// stored Sigma as the std image the reference left at ones) and the depth range the volume's bounds are planned from
// (sage_window_depth_range).  Both are opt-in: a window that never calls them launches what it did without them.
#include "runtime_internal.h"
#include "sage_device.h"

namespace
{

// grid: the listed keyframes' maps, [n][HW]; one writer per map.  out [n][2] = (minimum over the positive values, maximum) of
// the map with masked pixels read as 0; no positive value: minimum 0.  fminf / fmaxf: the same whatever the order
__global__ __launch_bounds__(kBlock) void depth_range_kernel(const float *__restrict__ dpt, const float *__restrict__ mask,
                                                           int HW, float *__restrict__ out)
{
  __shared__ float s_min[kBlock], s_max[kBlock];
  const int tid = threadIdx.x;
  const float *d = dpt + (size_t)blockIdx.x * HW;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < HW; i += kBlock)
  {
    const float v = (mask && mask[i] <= 0.5f) ? 0.0f : d[i];
    if (v > 0.0f)
      lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  s_min[tid] = lo;
  s_max[tid] = hi;
  __syncthreads();
  for (int step = kBlock / 2; step > 0; step >>= 1)
  {
    if (tid < step)
    {
      s_min[tid] = fminf(s_min[tid], s_min[tid + step]);
      s_max[tid] = fmaxf(s_max[tid], s_max[tid + step]);
    }
    __syncthreads();
  }
  if (tid == 0)
  {
    out[2 * blockIdx.x + 0] = s_min[0] == INFINITY ? 0.0f : s_min[0];
    out[2 * blockIdx.x + 1] = s_max[0];
  }
}

// what both calls refuse, or SAGE_OK: the arguments, a window that is not a finalized single-rank one
int tsdf_window_refusal(const SageWindow *w, const int32_t *kfs, int n)
{
  if (!w || !kfs || n < 1 || n > SAGE_TSDF_MAX_VIEWS)
    return SAGE_E_INVALID;
  if (!w->finalized)
    return SAGE_E_STATE;
  if (w->world > 1)
    return SAGE_E_UNSUPPORTED;
  if (w->cfg.CS != 16 && w->cfg.CS != 32)
    return SAGE_E_UNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (kfs[i] < 0 || kfs[i] >= w->K)
      return SAGE_E_INVALID;
  return SAGE_OK;
}

// the depth maps of the listed keyframes at the current variables into the window's TSDF scratch, [n][H * W] in the order
// given.  They are formed by the kernel of sage_depth_and_grad (one launch per keyframe, bias, basis, code and scale as the
// window's depth items name them), not by the window's depth batch: depth_batch_kernel contracts its dot product differently
// and gives other last bits, and a caller who fuses the same keyframes through sage_depth_and_grad and
// sage_tsdf_integrate_batch must get the same bytes.  The window's own maps and their bookkeeping are not touched
int tsdf_window_depth_maps(SageWindow *w, const int32_t *kfs, int n)
{
  const int H = (int)w->cfg.pyr.cam[0].h, W = (int)w->cfg.pyr.cam[0].w;
  if (const int rc = w->tsdf.depth.reserve((size_t)n * H * W * sizeof(float)))
    return rc;
  for (int i = 0; i < n; ++i)
  {
    const int k = kfs[i];
    const float *vp = w->vars[0].as<float>() + (size_t)k * w->VS;
    SAGE_HIP(launch_depth_and_grad(w->stream, w->cfg.CS, w->tsdf.depth.as<float>() + (size_t)i * H * W, nullptr, w->views[k].bias,
                                   w->views[k].basis, vp + 13, vp + 12, 0.f, H, W));
  }
  return SAGE_OK;
}

} // namespace

extern "C" int sage_window_depth_range(SageWindow *w, const int32_t *kfs, int n, float *dmin, float *dmax)
{
  if (!dmin || !dmax)
    return SAGE_E_INVALID;
  if (const int rc = tsdf_window_refusal(w, kfs, n))
    return rc;
  const int HW = (int)w->cfg.pyr.cam[0].h * (int)w->cfg.pyr.cam[0].w;
  int rc;
  if ((rc = w->tsdf.range.reserve((size_t)n * 2 * sizeof(float)))) // (every earlier call has drained the stream)
    return rc;
  float *out = w->tsdf.range.as<float>();
  if ((rc = tsdf_window_depth_maps(w, kfs, n)))
    return rc;
  hipLaunchKernelGGL(depth_range_kernel, dim3(n), dim3(kBlock), 0, w->stream, w->tsdf.depth.as<float>(), w->cfg.mask_dev, HW, out);
  SAGE_HIP(hipGetLastError());
  SAGE_HIP(hipStreamSynchronize(w->stream));
  float lo = INFINITY, hi = -INFINITY;
  for (int i = 0; i < n; ++i)
  {
    if (out[2 * i] > 0.0f)
      lo = std::fmin(lo, out[2 * i]);
    hi = std::fmax(hi, out[2 * i + 1]);
  }
  *dmin = lo == INFINITY ? 0.0f : lo;
  *dmax = hi;
  return SAGE_OK;
}

extern "C" int sage_window_fuse_tsdf(SageWindow *w, SageTsdfVolume *vol, const int32_t *kfs, int n, int std_mode, float std_floor,
                                     float obs_weight, float min_depth)
{
  if (!vol || (std_mode != SAGE_TSDF_STD_ONE && std_mode != SAGE_TSDF_STD_SIGMA))
    return SAGE_E_INVALID;
  if (const int rc = tsdf_window_refusal(w, kfs, n))
    return rc;
  if (std_mode == SAGE_TSDF_STD_SIGMA)
  {
    if (const int rc = covariance_refusal(w))
      return rc;
    if (!covariance_current(w))
      return SAGE_E_STATE;
  }
  const SageCamera &cam = w->cfg.pyr.cam[0];
  const int H = (int)cam.h, W = (int)cam.w, HW = H * W;
  std::vector<SageTsdfView> views((size_t)n);
  for (int i = 0; i < n; ++i)
  {
    SageTsdfView &v = views[i];
    std::memset(&v, 0, sizeof(v));
    v.depth_dev = w->vars[0].as<float>(); // (for the checks: the map's address is known once the scratch is)
    v.mask_dev = w->cfg.mask_dev;
    v.image_floats = HW;
    std::memcpy(v.pose12, &w->hv.pose[0][(size_t)kfs[i] * 12], 12 * sizeof(float));
    v.cam = cam;
    v.obs_weight = obs_weight; v.min_depth = min_depth; v.std_floor = std_floor;
  }
  int rc;
  if (std_mode == SAGE_TSDF_STD_SIGMA)
  {
    if ((rc = w->tsdf.sigma.reserve((size_t)n * HW * sizeof(float))))
      return rc;
    for (int i = 0; i < n; ++i)
      views[i].std_dev = w->tsdf.sigma.as<float>() + (size_t)i * HW;
  }
  if ((rc = sage::tsdf::check_batch(views.data(), n, 0))) // (before any launch)
    return rc;
  // the volume on the window's device?
  hipPointerAttribute_t pa_vol, pa_win;
  float *vol_tsdf = nullptr;
  (void)sage_tsdf_dev(vol, &vol_tsdf, nullptr, nullptr);
  SAGE_HIP(hipPointerGetAttributes(&pa_vol, vol_tsdf));
  SAGE_HIP(hipPointerGetAttributes(&pa_win, w->vars[0].p));
  if (pa_vol.device != pa_win.device)
    return SAGE_E_INVALID;
  if ((rc = tsdf_window_depth_maps(w, kfs, n)))
    return rc;
  for (int i = 0; i < n; ++i)
    views[i].depth_dev = w->tsdf.depth.as<float>() + (size_t)i * HW;
  if (std_mode == SAGE_TSDF_STD_SIGMA)
  {
    std::vector<DepthSigmaEntry> e((size_t)n);
    for (int i = 0; i < n; ++i)
      e[i] = window_sigma_entry(w, kfs[i], w->tsdf.sigma.as<float>() + (size_t)i * HW);
    if ((rc = depth_sigma_enqueue(w->stream, w->cov.stage, e.data(), n, H, W, w->cfg.CS, SAGE_DEPTH_SIGMA)))
      return rc;
  }
  return tsdf_integrate_batch_on(vol, w->stream, views.data(), n, 0);
}
