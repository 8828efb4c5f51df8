// keyframe_prepare.hip -- prepared keyframes (include/sage_ba.h "Prepared keyframes"): stages 3-5 of sage_window_finalize for B
// keyframes at once, outside any window, in launches that do not depend on B.  The two kernels restate repack_groups_kernel and
// presample_source_kernel (producers.hip) over a device table, expression for expression: a window built from handles holds
// the bytes its twin from views holds.  The location sort is producers.hip's own, already batched over keyframes.
// Host policy (fingerprint, checks, layouts, plan): keyframe_prepare_host.cpp.
#include "runtime_internal.h"
#include "sage_device.h"

#include <memory>

using sage::prep::PresampleItem;
using sage::prep::RepackItem;

static_assert(sizeof(SortItem) <= sage::prep::kSortItemBytes, "the scratch layout reserves kSortItemBytes per sort item");

// [FS][P] -> [FS/4][P][4] for the 3 B planes of a batch: grid (ceil(P / 256), FS / 4, 3 B), one f32x4 store per thread.
// Streaming: four coalesced dword loads (one per channel row), one coalesced 16-byte store, no LDS
__global__ __launch_bounds__(256) void repack_planes_batch_kernel(const RepackItem *__restrict__ items, int P, SagePyramid pyr,
                                                                  RepackScale ls)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (p >= P)
    return;
  const RepackItem it = items[blockIdx.z];
  const int axis = it.axis;
  int l = 0;
  for (int i = 1; i < pyr.levels; ++i)
    l = p >= pyr.level_offsets[i] ? i : l;
  float sc = axis == 0 ? 1.0f : (axis == 1 ? pyr.cam[l].fx : pyr.cam[l].fy);
  sc *= ls.s[l];
  const float *__restrict__ src = it.src;
  f32x4 v;
  v[0] = sc * src[(size_t)(4 * g + 0) * P + p];
  v[1] = sc * src[(size_t)(4 * g + 1) * P + p];
  v[2] = sc * src[(size_t)(4 * g + 2) * P + p];
  v[3] = sc * src[(size_t)(4 * g + 3) * P + p];
  *reinterpret_cast<f32x4 *>(it.dst + ((size_t)g * P + p) * 4) = v;
}

// f0s[l][g][n][0:4] = MINUS the 4-tap sample of the keyframe's own relaid feature plane at its sampled pixels, for the B
// keyframes of a batch: grid (ceil(max slots / 256), (FS / 4) L, B).  The tap expression is presample_source_kernel's
__global__ __launch_bounds__(256) void presample_source_batch_kernel(const PresampleItem *__restrict__ items, int G,
                                                                     const SagePyramid pyr, int exact_coord)
{
  const PresampleItem it = items[blockIdx.z];
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int l = blockIdx.y / G, g = blockIdx.y - l * G;
  const int N = it.slots;
  if (n >= N)
    return;
  const float *__restrict__ homo = it.homo;
  const float fx0 = pyr.cam[0].fx, fy0 = pyr.cam[0].fy, cx0 = pyr.cam[0].cx, cy0 = pyr.cam[0].cy;
  const float fxl = pyr.cam[l].fx, fyl = pyr.cam[l].fy;
  const int Wl = (int)pyr.cam[l].w, Hl = (int)pyr.cam[l].h;
  const float su = homo[3 * n + 0] * fx0 + cx0 + 0.5f, sv = homo[3 * n + 1] * fy0 + cy0 + 0.5f;
  Taps ts;
  if (exact_coord) // non-dyadic pyramid: the reference's own expression
    make_taps(ts, (su * fxl) / fx0 - 0.5f, (sv * fyl) / fy0 - 0.5f, Wl, Hl);
  else
    make_taps(ts, su * (fxl / fx0) - 0.5f, sv * (fyl / fy0) - 0.5f, Wl, Hl);
  const f32x4 *src = reinterpret_cast<const f32x4 *>(it.feat_pk) + (size_t)g * pyr.P + pyr.level_offsets[l];
  f32x4 f = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    f += ts.w[k] * src[ts.off[k]];
  reinterpret_cast<f32x4 *>(it.f0s)[((size_t)l * G + g) * N + n] = -f; // stored NEGATED, as the samplers read it
}

void prepared_retain(SagePreparedKeyframe *pk) { pk->refs.fetch_add(1, std::memory_order_relaxed); }

void prepared_release(SagePreparedKeyframe *pk)
{
  if (pk && pk->refs.fetch_sub(1, std::memory_order_acq_rel) == 1)
    delete pk; // (its allocation goes with its DevBuf)
}

extern "C" void sage_keyframe_release(SagePreparedKeyframe *pk) { prepared_release(pk); }

extern "C" int sage_keyframe_prepare_launches(const SageWorkspace *ws) { return ws ? ws->prep_launches : SAGE_E_INVALID; }

extern "C" int sage_keyframe_info(const SagePreparedKeyframe *pk, SagePreparedInfo *out)
{
  if (!pk || !out)
    return SAGE_E_INVALID;
  out->N = pk->view.N;
  out->slots = pk->slots;
  out->ordered = pk->ordered;
  out->padded = pk->padded;
  out->refs = pk->refs.load(std::memory_order_acquire);
  out->device_bytes = pk->lay.bytes;
  return SAGE_OK;
}

extern "C" int sage_keyframe_get(const SagePreparedKeyframe *pk, int what, void *host, size_t bytes)
{
  if (!pk || !host)
    return SAGE_E_INVALID;
  const SagePyramid &py = pk->fp.pyr;
  const void *src = nullptr;
  size_t n = 0;
  switch (what)
  {
  case SAGE_PREP_PACKED: src = pk->pk; n = (size_t)3 * pk->fp.FS * py.P * sizeof(float); break;
  case SAGE_PREP_LOC: src = pk->loc; n = (size_t)pk->slots * sizeof(int64_t); break;
  case SAGE_PREP_HOMO: src = pk->homo; n = (size_t)pk->slots * 3 * sizeof(float); break;
  case SAGE_PREP_F0S: src = pk->f0s; n = (size_t)py.levels * pk->fp.FS * pk->slots * sizeof(float); break;
  default: return SAGE_E_INVALID;
  }
  if (bytes != n)
    return SAGE_E_INVALID;
  if (n > 0)
    SAGE_HIP(hipMemcpy(host, src, n, hipMemcpyDeviceToHost));
  return SAGE_OK;
}

extern "C" int sage_keyframe_prepare_batch(SageWorkspace *ws, const SageWindowConfig *cfg, const SageKeyframeView *views, int B,
                                           SagePreparedKeyframe **out)
{
  if (out && B >= 1 && B <= SAGE_PREPARE_MAX_BATCH)
    for (int b = 0; b < B; ++b)
      out[b] = nullptr;
  if (ws)
    ws->prep_launches = 0; // (a refused call launches nothing)
  if (!ws ||!cfg || !views || !out || B < 1 || B > SAGE_PREPARE_MAX_BATCH)
    return SAGE_E_INVALID;
  int rc;
  if ((rc = prep::check_config(cfg)))
    return rc;
  for (int b = 0; b < B; ++b)
  {
    const SageKeyframeView &v = views[b];
    if (!v.feat_pyr || !v.grad_pyr || !v.bias || !v.basis || !v.loc1d || !v.homo || v.N < 0)
      return SAGE_E_INVALID;
  }
  const SagePyramid &py = cfg->pyr;
  const int FS = cfg->FS, G = FS / 4, L = py.levels, P = py.P;
  const int W = (int)py.cam[0].w, HW = (int)py.cam[0].h * W;
  const size_t plane_f = (size_t)FS * P;
  const prep::SampleSwitches sw = prep::sample_switches();
  const prep::Fingerprint fp = prep::fingerprint(*cfg, sw);
  hipStream_t s = ws->stream;

  // every allocation before any launch: a handle's from its N, the call's scratch from B and the image
  std::vector<std::unique_ptr<SagePreparedKeyframe>> hs(B);
  int max_n = 0;
  for (int b = 0; b < B; ++b)
  {
    hs[b].reset(new SagePreparedKeyframe());
    SagePreparedKeyframe &h = *hs[b];
    h.fp = fp;
    h.view = views[b];
    h.lay = prep::layout(FS, P, L, views[b].N);
    if ((rc = h.mem.reserve(h.lay.bytes)))
      return rc;
    max_n = std::max(max_n, views[b].N);
  }
  const prep::Scratch sc = prep::scratch(B, HW);
  if ((rc = ws->prep_scratch.reserve(sc.bytes)))
    return rc;
  char *const dev = ws->prep_scratch.as<char>();
  auto own = [&](int b, size_t off) { return hs[b]->mem.as<char>() + off; };

  // the tables: one host-to-device copy.  `host` outlives every copy out of it; whatever way the call ends, the stream is idle
  // before a handle that kernels write to is freed (the guard is declared last: it runs first)
  std::vector<char> host(sc.table_bytes, 0);
  std::vector<int> status((size_t)3 * B, 0), status2((size_t)2 * B, 0), pad_flags(B, 0); // status: [2 B] status | [B] tiles
  struct IdleOnExit
  {
    hipStream_t s;
    ~IdleOnExit() { (void)hipStreamSynchronize(s); }
  } idle{s};
  SortItem *sort_h = reinterpret_cast<SortItem *>(host.data() + sc.off_sort);
  RepackItem *rep_h = reinterpret_cast<RepackItem *>(host.data() + sc.off_repack);
  PresampleItem *pre_h = reinterpret_cast<PresampleItem *>(host.data() + sc.off_presample);
  for (int b = 0; b < B; ++b)
  {
    float *pk = reinterpret_cast<float *>(own(b, hs[b]->lay.off_pk));
    sort_h[b] = SortItem{reinterpret_cast<const long long *>(views[b].loc1d), views[b].homo,
                         reinterpret_cast<long long *>(own(b, hs[b]->lay.off_loc)),
                         reinterpret_cast<float *>(own(b, hs[b]->lay.off_homo)), views[b].N};
    rep_h[3 * b + 0] = RepackItem{pk, views[b].feat_pyr, 0, 0};
    rep_h[3 * b + 1] = RepackItem{pk + plane_f, views[b].grad_pyr, 1, 0};
    rep_h[3 * b + 2] = RepackItem{pk + 2 * plane_f, views[b].grad_pyr + plane_f, 2, 0};
  }
  SAGE_HIP(hipMemcpyAsync(dev + sc.off_sort, host.data(), sc.off_presample, hipMemcpyHostToDevice, s));

  // 1. the planes: every texel of level l carries its focal length (gradients) and sqrt(w_l), as finalize_pyramids folds them in
  RepackScale ls{};
  ls.on = 1;
  for (int l = 0; l < L; ++l)
    ls.s[l] = std::sqrt(cfg->photo_weights[l]);
  hipLaunchKernelGGL(repack_planes_batch_kernel, dim3((P + 255) / 256, G, 3 * B), dim3(256), 0, s,
                     reinterpret_cast<const RepackItem *>(dev + sc.off_repack), P, py, ls);
  SAGE_HIP(hipGetLastError());
  ws->prep_launches += 1;

  // 2. the samples: validated and relaid in tile order; 3. one wait for status and tile counts
  int *const status_dev = reinterpret_cast<int *>(dev + sc.off_status), *const tiles_dev = reinterpret_cast<int *>(dev + sc.off_tiles);
  int *const mark_dev = reinterpret_cast<int *>(dev + sc.off_mark), *const pad_dev = reinterpret_cast<int *>(dev + sc.off_pad);
  const SortItem *sort_dev = reinterpret_cast<const SortItem *>(dev + sc.off_sort);
  SAGE_HIP(launch_sort_locations(s, sort_dev, B, max_n, HW, mark_dev, status_dev, W, sw.tile_w, sw.tile_h, nullptr, tiles_dev));
  ws->prep_launches += max_n > 0 ? 4 : 3; // two fills, the mark pass, the ordering pass
  SAGE_HIP(hipMemcpyAsync(status.data(), status_dev, status.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  SAGE_HIP(hipStreamSynchronize(s));
  const int *tiles_nonempty = status.data() + 2 * B;
  for (int b = 0; b < B; ++b)
    if (status[2 * b] > 0)
      return SAGE_E_INVALID; // a location outside the image: no handle
  // 4. the tile-padded order, where finalize_samples would choose it: 8 x 8 tiles, not switched off, every sample kept,
  //    a partial tile, slots <= 1.25 x samples (which is what the allocation's cap holds)
  bool any_pad = false;
  for (int b = 0; b < B && sw.pad; ++b)
  {
    const long long slots = 64ll * tiles_nonempty[b], N = views[b].N;
    if (status[2 * b + 1] == N && slots > N && 4 * slots <= 5 * N)
      pad_flags[b] = 1, any_pad = true;
  }
  if (any_pad)
  {
    SAGE_HIP(hipMemcpyAsync(pad_dev, pad_flags.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    SAGE_HIP(launch_sort_locations(s, sort_dev, B, max_n, HW, mark_dev, status_dev, W, sw.tile_w, sw.tile_h, pad_dev, nullptr, true));
    ws->prep_launches += 1;
    SAGE_HIP(hipMemcpyAsync(status2.data(), status_dev, status2.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    SAGE_HIP(hipStreamSynchronize(s));
  }
  int max_slots = 0;
  for (int b = 0; b < B; ++b)
  {
    SagePreparedKeyframe &h = *hs[b];
    h.pk = reinterpret_cast<const float *>(own(b, h.lay.off_pk));
    h.f0s = reinterpret_cast<const float *>(own(b, h.lay.off_f0s));
    h.slots = views[b].N;
    if (pad_flags[b])
    {
      if (status2[2 * b + 1] != 64 * tiles_nonempty[b] || (size_t)status2[2 * b + 1] > h.lay.cap)
        return SAGE_E_STATE;
      h.slots = status2[2 * b + 1]; // holes included
      h.padded = 1;
    }
    h.ordered = status[2 * b + 1] == views[b].N ? 1 : 0; // (0: a pixel sampled twice -- the caller's order and arrays)
    h.loc = h.ordered ? reinterpret_cast<const int64_t *>(own(b, h.lay.off_loc)) : views[b].loc1d;
    h.homo = h.ordered ? reinterpret_cast<const float *>(own(b, h.lay.off_homo)) : views[b].homo;
    pre_h[b] = PresampleItem{const_cast<float *>(h.f0s), h.pk, h.homo, h.slots, 0};
    max_slots = std::max(max_slots, h.slots);
  }
  // 5. the negated source features; 6. the last wait
  if (max_slots > 0)
  {
    SAGE_HIP(hipMemcpyAsync(dev + sc.off_presample, pre_h, (size_t)B * sizeof(PresampleItem), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(presample_source_batch_kernel, dim3((max_slots + 255) / 256, G * L, B), dim3(256), 0, s,
                       reinterpret_cast<const PresampleItem *>(dev + sc.off_presample), G, py, pyramid_is_dyadic(py) ? 0 : 1);
    SAGE_HIP(hipGetLastError());
    ws->prep_launches += 1;
  }
  SAGE_HIP(hipStreamSynchronize(s));
  for (int b = 0; b < B; ++b)
    out[b] = hs[b].release();
  return SAGE_OK;
}

extern "C" int sage_keyframe_prepare(SageWorkspace *ws, const SageWindowConfig *cfg, const SageKeyframeView *view,
                                     SagePreparedKeyframe **out)
{
  return sage_keyframe_prepare_batch(ws, cfg, view, 1, out);
}
