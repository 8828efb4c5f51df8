// tsdf.hip -- TSDF fusion: TSDFVolume.integrate of representation/scripts/generate_reconstruction_fly_through.py:130-331, the
// stage that turns keyframe depth maps, poses and a per-pixel std image into the fused surface.  The specification, operation
// by operation, and where it departs from the reference's text are in include/sage_ba.h ("TSDF fusion"); tsdf_voxel below is
// the one definition both kernels run.
//
//   tsdf_integrate_kernel        one view: one thread per voxel, lanes along z (the three volume streams are coalesced).  The
//                                volume is read and written where the view reaches it: up to 24 bytes per voxel and view
//   tsdf_integrate_batch_kernel  n views in one launch.  A workgroup of 4 waves owns a brick of BX x 4 x 64 voxels: wave y of
//                                it owns the lines (x0 .. x0 + BX - 1, y0 + y, z0 .. z0 + 63), a lane one voxel of each: whole
//                                64-voxel lines are read and written.  A thread keeps its BX voxels' tsdf, weight and color in
//                                registers while it walks the views IN ORDER and writes them once at the end: 24 bytes per
//                                voxel whatever n.  The views' parameters (TsdfViewDev, 128 bytes) lie in a device table
//                                uploaded once per call; the workgroup stages them kViewChunk at a time in LDS (one 16-byte
//                                piece per thread), lane v of wave 0 tests view v against the brick (tsdf_view_reaches),
//                                a ballot orders the survivors, and all threads walk that list reading the parameters as
//                                LDS broadcasts.  A brick no view reaches is neither read nor written.
// No atomics, no waiting between workgroups; every output element has one writer and every loop a bound known at launch
// (the chunks of n, the views of a chunk, BX).  Per brick the kernel writes how many views it kept (one writer: not a counter).
//
// Byte for byte: the batch runs tsdf_voxel on the same inputs in the same order as n single launches do, fp contraction is
// off in it, division and roundf are correctly rounded and deterministic, and a voxel no view updates is written back as read.
#include "runtime_internal.h"
#include "sage_device.h"

using namespace sage::tsdf;

namespace
{

struct TsdfVolDev
{
  float *tsdf, *weight, *color; // color: null without a color volume
  int dx, dy, dz;
  float ox, oy, oz, voxel, trunc;
};

struct TsdfViewDev // a row of the batch's table: 128 bytes, 16-byte pieces
{
  float R[9], t[3];
  float fx, fy, cx, cy;
  const float *depth, *std, *mask, *color;
  int w, h;
  float obs_weight, min_depth, std_floor;
  int pad[3];
};
static_assert(sizeof(TsdfViewDev) == 128, "staged in LDS as 16-byte pieces, kViewChunk of them by 256 threads");
static_assert(kViewChunk * sizeof(TsdfViewDev) == 256 * 16 && kViewChunk <= 64, "one piece per thread; the cull is one wave's");

TsdfViewDev view_dev(const SageTsdfView &v)
{
  TsdfViewDev d;
  std::memset(&d, 0, sizeof(d));
  std::memcpy(d.R, v.pose12, 9 * sizeof(float));
  std::memcpy(d.t, v.pose12 + 9, 3 * sizeof(float));
  d.fx = v.cam.fx; d.fy = v.cam.fy; d.cx = v.cam.cx; d.cy = v.cam.cy;
  d.depth = v.depth_dev; d.std = v.std_dev; d.mask = v.mask_dev; d.color = v.color_dev;
  d.w = (int)v.cam.w; d.h = (int)v.cam.h;
  d.obs_weight = v.obs_weight; d.min_depth = v.min_depth; d.std_floor = v.std_floor;
  return d;
}

// step 1 for one axis
__device__ __forceinline__ float tsdf_coord(float origin, int i, float voxel)
{
#pragma clang fp contract(off)
  const float s = (float)i * voxel;
  return origin + s;
}

// steps 2-11 for the voxel at p: tsdf, weight and color in and out (color is read and written only with a color image)
__device__ __forceinline__ void tsdf_voxel(const TsdfViewDev &V, float trunc, float px, float py, float pz, float &tsdf, float &weight,
                                           float &color)
{
#pragma clang fp contract(off)
  const float qx = px - V.t[0], qy = py - V.t[1], qz = pz - V.t[2];
  const float cz = (V.R[2] * qx + V.R[5] * qy) + V.R[8] * qz;
  if (cz < V.min_depth)
    return;
  const float cx = (V.R[0] * qx + V.R[3] * qy) + V.R[6] * qz;
  const float cy = (V.R[1] * qx + V.R[4] * qy) + V.R[7] * qz;
  const float ru = roundf(V.fx * (cx / cz) + V.cx), rv = roundf(V.fy * (cy / cz) + V.cy);
  // (the test in float: the same pixels as the integers' wherever the conversion is defined; a NaN skips)
  if (!(ru >= 0.0f && ru < (float)V.w && rv >= 0.0f && rv < (float)V.h))
    return;
  const int at = (int)rv * V.w + (int)ru;
  float d = V.depth[at];
  if (V.mask && V.mask[at] <= 0.5f)
    d = 0.0f;
  float s = V.std ? V.std[at] : 1.0f;
  s = fmaxf(s, V.std_floor);
  if (d <= 0.0f || s <= 0.0f)
    return;
  const float diff = d - cz;
  if (diff < -trunc)
    return;
  const float dist = fminf(1.0f, diff / s);
  const float w_old = weight, ow = V.obs_weight;
  const float w_new = w_old + ow;
  tsdf = (tsdf * w_old + dist * ow) / w_new;
  weight = w_new;
  if (V.color)
  {
    const float nc = V.color[at];
    float nb = floorf(nc / 65536.0f);
    float ng = floorf((nc - nb * 65536.0f) / 256.0f);
    float nr = nc - nb * 65536.0f - ng * 256.0f;
    const float oc = color;
    const float ob = floorf(oc / 65536.0f);
    const float og = floorf((oc - ob * 65536.0f) / 256.0f);
    const float orr = oc - ob * 65536.0f - og * 256.0f;
    nb = fminf(roundf((ob * w_old + nb * ow) / w_new), 255.0f);
    ng = fminf(roundf((og * w_old + ng * ow) / w_new), 255.0f);
    nr = fminf(roundf((orr * w_old + nr * ow) / w_new), 255.0f);
    color = nb * 65536.0f + ng * 256.0f + nr;
  }
}

__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(const TsdfVolDev G, const TsdfViewDev V)
{
  const long long idx = (long long)blockIdx.x * kBlock + threadIdx.x; // integer arithmetic, < N (deviation (i))
  const long long N = (long long)G.dx * G.dy * G.dz;
  if (idx >= N)
    return;
  const int plane = G.dy * G.dz; // (N < 2^31)
  const int ix = (int)(idx / plane), rem = (int)(idx - (long long)ix * plane), iy = rem / G.dz, iz = rem - iy * G.dz;
  const float px = tsdf_coord(G.ox, ix, G.voxel), py = tsdf_coord(G.oy, iy, G.voxel), pz = tsdf_coord(G.oz, iz, G.voxel);
  const bool col = V.color != nullptr;
  const float t0 = G.tsdf[idx], w0 = G.weight[idx], c0 = col ? G.color[idx] : 0.0f;
  float t = t0, w = w0, c = c0;
  tsdf_voxel(V, G.trunc, px, py, pz, t, w, c);
  if (w != w0 || t != t0) // (an update raises the weight by obs_weight > 0; a weight too large to rise takes no part in the test)
  {
    G.tsdf[idx] = t;
    G.weight[idx] = w;
  }
  if (col && c != c0)
    G.color[idx] = c;
}

// Can a voxel of the brick [x0, x1] x [y0, y1] x [z0, z1] (voxel indices, inclusive) pass steps 4-6 of view V?  false only when
// none can.  With F the exact affine map from the voxel index to camera coordinates (fp32 parameters, real arithmetic), a voxel
// passes the left side only if  fx c_x + (cx + 0.5) c_z > -slack  for its COMPUTED c, and |c - F| <= E: so when the plane
// function of F lies below -slack at all eight corners (it is affine: its extremes over the brick are at corners) no voxel
// passes.  Likewise the right, top and bottom sides and c_z >= min_depth.  E = 8 u Rmax (m_x + m_y + m_z), u = 2^-24, m_a the
// largest |origin_a| + |i voxel| + |t_a| of the brick: 3 roundings in q, 3 in the dot product.  The side planes hold for
// c_z > 0 only (they are the pixel tests multiplied by c_z): they are used when min_depth > 0.  slack, per side with k the
// coefficient of c_z:  4 [(f + |k|) E + u (2 f + max(w, h)) Cmax],  Cmax the largest |F| + E at a corner: the first term
// moves c to F, the second covers the roundings of the division, the product and the sum; 4 is a margin over the terms of
// second order.  DESIGN.md s3 "TSDF fusion" has the derivation.  A NaN anywhere compares false: the view is kept.
__device__ bool tsdf_view_reaches(const TsdfVolDev &G, const TsdfViewDev &V, int x0, int x1, int y0, int y1, int z0, int z1)
{
  const double u = 5.9604644775390625e-08, vox = (double)G.voxel;
  const double o[3] = {(double)G.ox, (double)G.oy, (double)G.oz};
  const int lo[3] = {x0, y0, z0}, hi[3] = {x1, y1, z1};
  double m = 0.0, rmax = 0.0;
  for (int a = 0; a < 3; ++a)
    m += fabs(o[a]) + fabs((double)hi[a] * vox) + fabs((double)V.t[a]);
  for (int i = 0; i < 9; ++i)
    rmax = fmax(rmax, fabs((double)V.R[i]));
  const double E = 8.0 * u * rmax * m;
  const double fx = (double)V.fx, fy = (double)V.fy;
  const double kl = (double)V.cx + 0.5, kr = (double)V.cx - (double)V.w + 0.5, kt = (double)V.cy + 0.5, kb = (double)V.cy - (double)V.h + 0.5;
  double zmax = -INFINITY, lmax = -INFINITY, rmin = INFINITY, tmax = -INFINITY, bmin = INFINITY, cmax = 0.0;
  for (int corner = 0; corner < 8; ++corner)
  {
    double q[3];
    for (int a = 0; a < 3; ++a)
      q[a] = (o[a] + (double)((corner >> a) & 1 ? hi[a] : lo[a]) * vox) - (double)V.t[a];
    const double cx = (double)V.R[0] * q[0] + (double)V.R[3] * q[1] + (double)V.R[6] * q[2];
    const double cy = (double)V.R[1] * q[0] + (double)V.R[4] * q[1] + (double)V.R[7] * q[2];
    const double cz = (double)V.R[2] * q[0] + (double)V.R[5] * q[1] + (double)V.R[8] * q[2];
    zmax = fmax(zmax, cz);
    lmax = fmax(lmax, fx * cx + kl * cz);
    rmin = fmin(rmin, fx * cx + kr * cz);
    tmax = fmax(tmax, fy * cy + kt * cz);
    bmin = fmin(bmin, fy * cy + kb * cz);
    cmax = fmax(cmax, fmax(fabs(cx), fmax(fabs(cy), fabs(cz))));
  }
  cmax += E;
  if (zmax < (double)V.min_depth - 4.0 * E)
    return false;
  if (!(V.min_depth > 0.0f))
    return true;
  const double wh = fmax((double)V.w, (double)V.h);
  const double rx = u * (2.0 * fx + wh) * cmax, ry = u * (2.0 * fy + wh) * cmax;
  if (lmax < -4.0 * ((fx + fabs(kl)) * E + rx) || rmin > 4.0 * ((fx + fabs(kr)) * E + rx))
    return false;
  if (tmax < -4.0 * ((fy + fabs(kt)) * E + ry) || bmin > 4.0 * ((fy + fabs(kb)) * E + ry))
    return false;
  return true;
}

template <int BX>
__global__ __launch_bounds__(kBlock) void tsdf_integrate_batch_kernel(const TsdfVolDev G, const TsdfViewDev *__restrict__ views, int n,
                                                                      int no_cull, int nby, int nbz, int32_t *__restrict__ kept_out)
{
  __shared__ __attribute__((aligned(16))) TsdfViewDev s_view[kViewChunk];
  __shared__ int s_list[kViewChunk];
  __shared__ int s_count;
  static_assert(kBlock == kBrickY * kBrickZ && kBrickZ == 64, "a wave per line, a lane per voxel of it");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, bz = b % nbz, by = (b / nbz) % nby, bx = b / (nbz * nby);
  const int x0 = bx * BX, y0 = by * kBrickY, z0 = bz * kBrickZ;
  const int x1 = min(x0 + BX, G.dx) - 1, y1 = min(y0 + kBrickY, G.dy) - 1, z1 = min(z0 + kBrickZ, G.dz) - 1;
  const int iy = y0 + wave, iz = z0 + lane;
  const bool line = iy < G.dy && iz < G.dz;
  const float py = tsdf_coord(G.oy, iy, G.voxel), pz = tsdf_coord(G.oz, iz, G.voxel);
  float px[BX], t[BX], w[BX], c[BX];
  long long at[BX];
  bool live[BX];
#pragma unroll
  for (int j = 0; j < BX; ++j)
  {
    live[j] = line && x0 + j < G.dx;
    at[j] = ((long long)(x0 + j) * G.dy + iy) * G.dz + iz;
    px[j] = tsdf_coord(G.ox, x0 + j, G.voxel);
    t[j] = w[j] = c[j] = 0.0f;
  }
  bool loaded = false; // (uniform over the workgroup)
  int kept = 0;
  for (int v0 = 0; v0 < n; v0 += kViewChunk)
  {
    const int nv = min(kViewChunk, n - v0);
    __syncthreads(); // (the walk of the chunk before has read s_view and s_list)
    if (tid < nv * 8) // 8 pieces of 16 bytes per view
      reinterpret_cast<f32x4 *>(s_view)[tid] = reinterpret_cast<const f32x4 *>(views + v0)[tid];
    __syncthreads();
    if (wave == 0)
    {
      const bool mine = lane < nv && (no_cull || tsdf_view_reaches(G, s_view[lane], x0, x1, y0, y1, z0, z1));
      const unsigned long long m = __ballot(mine);
      if (mine)
        s_list[__popcll(m & ((1ull << lane) - 1ull))] = lane; // ascending: the order given
      if (lane == 0)
        s_count = __popcll(m);
    }
    __syncthreads();
    const int cnt = s_count;
    if (cnt == 0)
      continue;
    kept += cnt;
    if (!loaded)
    {
      loaded = true;
#pragma unroll
      for (int j = 0; j < BX; ++j)
        if (live[j])
        {
          t[j] = G.tsdf[at[j]];
          w[j] = G.weight[at[j]];
          c[j] = G.color ? G.color[at[j]] : 0.0f;
        }
    }
    for (int i = 0; i < cnt; ++i)
    {
      const TsdfViewDev &V = s_view[s_list[i]];
#pragma unroll
      for (int j = 0; j < BX; ++j)
        if (live[j])
          tsdf_voxel(V, G.trunc, px[j], py, pz, t[j], w[j], c[j]);
    }
  }
  if (loaded)
  {
#pragma unroll
    for (int j = 0; j < BX; ++j)
      if (live[j])
      {
        G.tsdf[at[j]] = t[j];
        G.weight[at[j]] = w[j];
        if (G.color)
          G.color[at[j]] = c[j];
      }
  }
  if (tid == 0)
    kept_out[b] = kept;
}

TsdfVolDev vol_dev(const SageTsdfVolume *vol)
{
  const SageTsdfPlan &p = vol->plan;
  return TsdfVolDev{vol->tsdf.as<float>(), vol->weight.as<float>(), vol->color.as<float>(), p.dim[0], p.dim[1], p.dim[2],
                    p.origin[0], p.origin[1], p.origin[2], p.voxel_size, p.trunc_margin};
}

} // namespace

extern "C" int sage_tsdf_create(SageWorkspace *ws, const SageTsdfPlan *plan, SageTsdfVolume **out)
{
  if (!ws || !plan || !out)
    return SAGE_E_INVALID;
  *out = nullptr;
  const SageTsdfPlan &p = *plan;
  if (p.dim[0] < 1 || p.dim[1] < 1 || p.dim[2] < 1 || (double)p.dim[0] * p.dim[1] * p.dim[2] > 2147483647.0 ||
      p.voxels != (int64_t)p.dim[0] * p.dim[1] * p.dim[2] || !std::isfinite(p.voxel_size) || !(p.voxel_size > 0.f) ||
      !std::isfinite(p.trunc_margin) || !(p.trunc_margin > 0.f) || !std::isfinite(p.origin[0]) || !std::isfinite(p.origin[1]) ||
      !std::isfinite(p.origin[2]))
    return SAGE_E_INVALID;
  SageTsdfVolume *vol = new SageTsdfVolume();
  vol->ws = ws;
  vol->plan = p;
  const size_t bytes = (size_t)p.voxels * sizeof(float);
  int rc;
  if ((rc = vol->tsdf.reserve(bytes)) || (rc = vol->weight.reserve(bytes)) || (p.with_color && (rc = vol->color.reserve(bytes))) ||
      (rc = vol->kept.reserve((size_t)bricks_of(p.dim, 1) * sizeof(int32_t))) ||
      (rc = (int)hipEventCreateWithFlags(&vol->order, hipEventDisableTiming)) || (rc = sage_tsdf_reset(vol)))
  {
    sage_tsdf_destroy(vol);
    return rc;
  }
  *out = vol;
  return SAGE_OK;
}

extern "C" void sage_tsdf_destroy(SageTsdfVolume *vol)
{
  if (!vol)
    return;
  if (vol->ws)
    (void)hipStreamSynchronize(vol->ws->stream);
  if (vol->order)
    (void)hipEventDestroy(vol->order);
  delete vol;
}

extern "C" int sage_tsdf_reset(SageTsdfVolume *vol)
{
  if (!vol)
    return SAGE_E_INVALID;
  hipStream_t s = vol->ws->stream;
  const size_t bytes = (size_t)vol->plan.voxels * sizeof(float);
  SAGE_HIP(hipMemsetAsync(vol->tsdf.p, 0, bytes, s));
  SAGE_HIP(hipMemsetAsync(vol->weight.p, 0, bytes, s));
  if (vol->color.p)
    SAGE_HIP(hipMemsetAsync(vol->color.p, 0, bytes, s));
  return SAGE_OK;
}

extern "C" int sage_tsdf_get(SageTsdfVolume *vol, float *tsdf, float *weight, float *color)
{
  if (!vol || (color && !vol->color.p))
    return SAGE_E_INVALID;
  hipStream_t s = vol->ws->stream;
  const size_t bytes = (size_t)vol->plan.voxels * sizeof(float);
  if (tsdf)
    SAGE_HIP(hipMemcpyAsync(tsdf, vol->tsdf.p, bytes, hipMemcpyDeviceToHost, s));
  if (weight)
    SAGE_HIP(hipMemcpyAsync(weight, vol->weight.p, bytes, hipMemcpyDeviceToHost, s));
  if (color)
    SAGE_HIP(hipMemcpyAsync(color, vol->color.p, bytes, hipMemcpyDeviceToHost, s));
  SAGE_HIP(hipStreamSynchronize(s));
  return SAGE_OK;
}

extern "C" int sage_tsdf_dev(SageTsdfVolume *vol, float **tsdf, float **weight, float **color)
{
  if (!vol)
    return SAGE_E_INVALID;
  if (tsdf)
    *tsdf = vol->tsdf.as<float>();
  if (weight)
    *weight = vol->weight.as<float>();
  if (color)
    *color = vol->color.as<float>();
  return SAGE_OK;
}

extern "C" int sage_tsdf_integrate(SageTsdfVolume *vol, const SageTsdfView *view)
{
  if (!vol || !view)
    return SAGE_E_INVALID;
  if (const int rc = check_view(view))
    return rc;
  if (view->color_dev && !vol->color.p)
    return SAGE_E_INVALID;
  const unsigned blocks = (unsigned)(((long long)vol->plan.voxels + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(blocks), dim3(kBlock), 0, vol->ws->stream, vol_dev(vol), view_dev(*view));
  SAGE_HIP(hipGetLastError());
  return SAGE_OK;
}

int tsdf_integrate_batch_on(SageTsdfVolume *vol, hipStream_t s, const SageTsdfView *views, int n, int flags)
{
  for (int i = 0; i < n; ++i)
    if (views[i].color_dev && !vol->color.p)
      return SAGE_E_INVALID;
  SageWorkspace *ws = vol->ws;
  DepthSigmaStage &stage = ws->tsdf_stage;
  const size_t bytes = (size_t)n * sizeof(TsdfViewDev);
  int rc;
  if (stage.busy) // the last call's copy has left the pinned side?
    SAGE_HIP(hipEventSynchronize(stage.copied));
  stage.busy = false;
  if ((rc = stage.host.reserve((size_t)kMaxViews * sizeof(TsdfViewDev))) || (rc = stage.dev.reserve((size_t)kMaxViews * sizeof(TsdfViewDev))))
    return rc;
  if (!stage.copied)
    SAGE_HIP(hipEventCreateWithFlags(&stage.copied, hipEventDisableTiming));
  TsdfViewDev *table = stage.host.as<TsdfViewDev>();
  for (int i = 0; i < n; ++i)
    table[i] = view_dev(views[i]);
  const bool foreign = s != ws->stream;
  if (foreign) // s behind whatever the volume's stream holds
  {
    SAGE_HIP(hipEventRecord(vol->order, ws->stream));
    SAGE_HIP(hipStreamWaitEvent(s, vol->order, 0));
  }
  SAGE_HIP(hipMemcpyAsync(stage.dev.p, stage.host.p, bytes, hipMemcpyHostToDevice, s));
  SAGE_HIP(hipEventRecord(stage.copied, s));
  stage.busy = true;
  const int brick_x = brick_x_of(flags);
  const int32_t *dim = vol->plan.dim;
  const int nby = (dim[1] + kBrickY - 1) / kBrickY, nbz = (dim[2] + kBrickZ - 1) / kBrickZ;
  const unsigned bricks = (unsigned)bricks_of(dim, brick_x);
  const TsdfVolDev G = vol_dev(vol);
  const TsdfViewDev *tab = stage.dev.as<TsdfViewDev>();
  const int no_cull = (flags & SAGE_TSDF_NO_CULL) ? 1 : 0;
  int32_t *kept = vol->kept.as<int32_t>();
  if (brick_x == 1)
    hipLaunchKernelGGL((tsdf_integrate_batch_kernel<1>), dim3(bricks), dim3(kBlock), 0, s, G, tab, n, no_cull, nby, nbz, kept);
  else if (brick_x == 2)
    hipLaunchKernelGGL((tsdf_integrate_batch_kernel<2>), dim3(bricks), dim3(kBlock), 0, s, G, tab, n, no_cull, nby, nbz, kept);
  else
    hipLaunchKernelGGL((tsdf_integrate_batch_kernel<4>), dim3(bricks), dim3(kBlock), 0, s, G, tab, n, no_cull, nby, nbz, kept);
  SAGE_HIP(hipGetLastError());
  vol->last_views = n;
  vol->last_brick_x = brick_x;
  if (foreign) // the volume's stream behind the launch
  {
    SAGE_HIP(hipEventRecord(vol->order, s));
    SAGE_HIP(hipStreamWaitEvent(ws->stream, vol->order, 0));
  }
  return SAGE_OK;
}

extern "C" int sage_tsdf_integrate_batch(SageTsdfVolume *vol, const SageTsdfView *views, int n, int flags)
{
  if (!vol)
    return SAGE_E_INVALID;
  if (const int rc = check_batch(views, n, flags))
    return rc;
  return tsdf_integrate_batch_on(vol, vol->ws->stream, views, n, flags);
}

extern "C" int sage_tsdf_last_stats(SageTsdfVolume *vol, SageTsdfStats *out)
{
  if (!vol || !out)
    return SAGE_E_INVALID;
  if (vol->last_views == 0)
    return SAGE_E_STATE;
  const long long bricks = bricks_of(vol->plan.dim, vol->last_brick_x);
  std::vector<int32_t> kept((size_t)bricks);
  SAGE_HIP(hipMemcpyAsync(kept.data(), vol->kept.p, (size_t)bricks * sizeof(int32_t), hipMemcpyDeviceToHost, vol->ws->stream));
  SAGE_HIP(hipStreamSynchronize(vol->ws->stream));
  SageTsdfStats st{};
  st.bricks = bricks;
  st.views = vol->last_views;
  st.pairs = bricks * vol->last_views;
  for (int32_t k : kept)
    st.pairs_kept += k;
  st.brick[0] = vol->last_brick_x; st.brick[1] = kBrickY; st.brick[2] = kBrickZ;
  *out = st;
  return SAGE_OK;
}
