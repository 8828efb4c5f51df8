// window.hip -- the batched window engine on a finalized window (built by window_build.hip): deterministic assembly into
// block-sparse normal equations, linearize / error pass / damped solve / LM iteration (no reference counterpart: SURVEY s8 "new").
#include "runtime_internal.h"
#include "finalize_bodies.h"

namespace sage
{

// B-index (0..6+CS: pose 6, code CS, scale) -> column of the per-edge system, or -1 if absent
__device__ __forceinline__ int edge_col(int type, int role, int bi, int CS)
{
  if (bi < 6)
    return role * 6 + bi;
  if (type == 0)
  {
    if (role == 1)
      return -1; // a photometric edge does not touch code1 / scale1
    return bi < 6 + CS ? 12 + (bi - 6) : 12 + CS;
  }
  if (bi < 6 + CS)
    return 12 + role * CS + (bi - 6);
  return 12 + 2 * CS + role;
}

// one workgroup per output block; thread per element; contributions summed in a fixed order (deterministic)
// KP: the window carries keypoint terms (AdjEntry::type 2 / 3, the link lists, their share of the tail); windows without them
// run the instantiation that knows nothing of them
template <bool KP>
__global__ __launch_bounds__(1024) void assemble_kernel(const AssembleParams p)
{
  const int B = 7 + p.CS, BB = B * B;
  const int Dp = 13 + p.CS, Dg = 14 + 2 * p.CS;
  const int split = p.split > 1 ? p.split : 1;
  const int part = (int)blockIdx.x % split, bslot = (int)blockIdx.x / split;
  const int blk = p.blocks ? p.blocks[bslot] : bslot;
  const int tstride = (int)blockDim.x * split, tfirst = part * (int)blockDim.x + (int)threadIdx.x; // element striding
  double *diag = p.packed;
  double *lnk = diag + (size_t)p.K * BB;
  double *g = lnk + (size_t)p.nlinks * BB;
  double *tail = g + (size_t)p.K * B;
  if (blk < p.K)
  {
    // fp64 accumulation of the fp32 per-edge results (the reference widens to double before gtsam sums them:
    // photometric_factor.cpp:305-306).  Adjacency loop outside, the lane's (at most two) outputs inside: the gathers of
    // different adjacency entries are independent, so they overlap instead of forming one chain of ~150 dependent loads
    const int k = blk;
    const int a0 = p.adj_start[k], a1 = p.adj_start[k + 1];
    constexpr int S = 2;
    for (int base = 0; base < BB + B; base += S * tstride) // one pass with 1024 threads (or 4 x 256)
    {
    double acc[S] = {0.0, 0.0};
    int bi[S], bj[S];
    bool isg[S], valid[S];
#pragma unroll
    for (int s = 0; s < S; ++s)
    {
      const int idx = base + tfirst + s * tstride;
      valid[s] = idx < BB + B;
      isg[s] = idx >= BB;
      bi[s] = isg[s] ? idx - BB : idx / B;
      bj[s] = isg[s] ? 0 : idx % B;
    }
#pragma unroll 4
    for (int a = a0; a < a1; ++a)
    {
      const AdjEntry ae = p.adj[a];
      const int lt = KP ? (ae.type & 1) : ae.type; // column map: keypoint terms (types 2 / 3) share the dense layouts
      const bool kp = KP && ae.type >= 2;
      const int D = lt == 0 ? Dp : Dg;
      const float *A = kp ? (lt == 0 ? p.AtA_kr : p.AtA_km) : (lt == 0 ? p.AtA_p : p.AtA_g);
      const float *b = kp ? (lt == 0 ? p.Atb_kr : p.Atb_km) : (lt == 0 ? p.Atb_p : p.Atb_g);
#pragma unroll
      for (int s = 0; s < S; ++s)
      {
        if (!valid[s])
          continue;
        const int ci = edge_col(lt, ae.role, bi[s], p.CS);
        const int cj = isg[s] ? 0 : edge_col(lt, ae.role, bj[s], p.CS);
        if (ci < 0 || cj < 0)
          continue;
        const double *Wd = kp ? nullptr : (lt == 0 ? p.wide_p : p.wide_g);
        if (Wd)
          acc[s] += Wd[(size_t)ae.edge * (D * D + D) + (isg[s] ? (size_t)D * D + ci : (size_t)ci * D + cj)];
        else
          acc[s] += isg[s] ? (double)b[(size_t)ae.edge * D + ci] : (double)A[(size_t)ae.edge * D * D + (size_t)ci * D + cj];
      }
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
    {
      const int idx = base + tfirst + s * tstride;
      if (!valid[s])
        continue;
      if (isg[s])
        g[(size_t)k * B + bi[s]] = acc[s];
      else
        diag[(size_t)k * BB + idx] = acc[s];
    }
    } // passes
  }
  else if (blk < p.K + p.nlinks)
  {
    const int l = blk - p.K;
    const LinkEdges le = p.links[l];
    for (int idx = tfirst; idx < BB; idx += tstride)
    {
      const int bi = idx / B, bj = idx % B; // bi indexes keyframe a (older), bj keyframe b
      double acc = 0.0;
      {
        for (int type = 0; type < 2; ++type)
        {
          if ((type == 0 && !p.AtA_p) || (type == 1 && !p.AtA_g))
            continue;
          const int D = type == 0 ? Dp : Dg;
          const float *A = type == 0 ? p.AtA_p : p.AtA_g;
          const double *Wd = type == 0 ? p.wide_p : p.wide_g;
          const size_t ws = (size_t)D * D + D;
          // edge a->b : a has role 0, b has role 1
          int ci = edge_col(type, 0, bi, p.CS), cj = edge_col(type, 1, bj, p.CS);
          if (le.e_ab >= 0 && ci >= 0 && cj >= 0) // (each direction on its own: the other one may belong to another rank)
            acc += Wd ? Wd[(size_t)le.e_ab * ws + (size_t)ci * D + cj] : (double)A[(size_t)le.e_ab * D * D + (size_t)ci * D + cj];
          // edge b->a : b has role 0, a has role 1
          ci = edge_col(type, 1, bi, p.CS);
          cj = edge_col(type, 0, bj, p.CS);
          if (le.e_ba >= 0 && ci >= 0 && cj >= 0)
            acc += Wd ? Wd[(size_t)le.e_ba * ws + (size_t)ci * D + cj] : (double)A[(size_t)le.e_ba * D * D + (size_t)ci * D + cj];
        }
      }
      if (KP && p.link_kp_start) // keypoint terms of the link's two directions, in the order they were added (per kind)
        for (int a = p.link_kp_start[l]; a < p.link_kp_start[l + 1]; ++a)
        {
          const AdjEntry ae = p.link_kp[a];
          const int lt = ae.type & 1, D = lt == 0 ? Dp : Dg;
          const float *A = lt == 0 ? p.AtA_kr : p.AtA_km;
          const int ci = edge_col(lt, ae.role, bi, p.CS), cj = edge_col(lt, 1 - ae.role, bj, p.CS); // (role = direction)
          if (ci >= 0 && cj >= 0)
            acc += (double)A[(size_t)ae.edge * D * D + (size_t)ci * D + cj];
        }
      lnk[(size_t)l * BB + idx] = acc;
    }
  }
  else
  {
    // tail: total errors / inlier counts of the local edges; one wave per sum, fixed lane order (deterministic)
    if (part != 0)
      return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool photo = (wave & 1) == 0;
    const int which = wave >> 1; // 0: error, 1: inliers
    const float *st = photo ? p.stats_p : p.stats_g;
    const int n = photo ? p.n_edges_p : p.n_edges_g;
    double acc = 0.0;
    if (st && wave < 4)
      for (int e = lane; e < n; e += 64)
        acc += (double)st[2 * e + which];
    if (KP && p.stats_k && wave < 2) // the terms' errors: reprojection in the photometric slot, match geometry in the geometric one
    {
      const float *sk = p.stats_k + (photo ? 0 : 2 * (size_t)p.n_kr);
      const int nk = photo ? p.n_kr : p.n_km;
      for (int t = lane; t < nk; t += 64)
        acc += (double)sk[2 * t];
    }
    for (int off = 32; off > 0; off >>= 1)
      acc += __shfl_down(acc, off);
    if (lane == 0 && wave < 4)
    {
      tail[which * 2 + (photo ? 0 : 1)] = acc; // [err_photo err_geo n_photo n_geo]
      if (p.tail_mirror)
        p.tail_mirror[which * 2 + (photo ? 0 : 1)] = acc;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// per-edge finalize of BOTH factor types in one launch (a workgroup per edge and type): the geometric finalize no longer
// sits between the two big kernels (18 us + a launch gap on the step's critical path, r04 timeline)
// ------------------------------------------------------------------------------------------------
struct WindowFinalizeParams
{
  PhotoFinalizeParams ph;
  GeoFinalizeParams ge;
  int n_p, n_g;
};

template <int CS>
__global__ __launch_bounds__(kFinalizeBlock) void window_finalize_kernel(const WindowFinalizeParams prm)
{
  constexpr int LDS = photo_finalize_lds_doubles(CS) > geo_finalize_lds_doubles(CS) ? photo_finalize_lds_doubles(CS)
                                                                                    : geo_finalize_lds_doubles(CS);
  __shared__ double s[LDS];
  const int bid = (int)blockIdx.x;
  if (bid < prm.n_g) // (the longer finalize first)
    geo_finalize_body<CS>(prm.ge, bid, s);
  else
    photo_finalize_body<CS>(prm.ph, bid - prm.n_g, s);
}

// error pass of a window in ONE tail kernel: per-edge statistics of both factor types from the workgroup partials
// (what stats_finalize_kernel does: photometric_factor_kernels.cpp:1049-1058, geometric :868-878) and their totals
// (a wave-parallel sum in a fixed lane order) -- same summation orders, three launches and their gaps less on the step's critical path.

template <bool KP>
__global__ __launch_bounds__(1024) void error_totals_kernel(const ErrorTotalsSide ph, const ErrorTotalsSide ge, double *out,
                                                            double *mirror, double epoch, const KpTotals kp)
{
  for (int idx = threadIdx.x; idx < ph.n_edges + ge.n_edges; idx += blockDim.x)
  {
    const bool photo = idx < ph.n_edges;
    const ErrorTotalsSide &sd = photo ? ph : ge;
    const int e = photo ? idx : idx - ph.n_edges;
    const int first = sd.edge_first[e], nt = sd.edge_tiles[e];
    // same order of the sums as stats_finalize_kernel; eight records' loads in flight at a time (a chain of dependent
    // cache misses otherwise: this one-workgroup kernel sits on the step's critical path)
    float se = 0.f, sn = 0.f;
    for (int t0 = 0; t0 < nt; t0 += 8)
    {
      float ve[8], vn[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
      {
        const int t = t0 + u < nt ? t0 + u : nt - 1;
        ve[u] = sd.partials[(size_t)(first + t) * sd.stride + sd.err_off];
        vn[u] = sd.partials[(size_t)(first + t) * sd.stride + sd.cnt_off];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t0 + u < nt)
        {
          se += ve[u];
          sn += vn[u];
        }
    }
    sd.stats[2 * e + 0] = sn > 0.f ? sd.scale * se / sn : sd.fallback;
    sd.stats[2 * e + 1] = sn;
  }
  __threadfence_block();
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave >= 4)
    return;
  const bool photo = (wave & 1) == 0;
  const int which = wave >> 1;
  const ErrorTotalsSide &sd = photo ? ph : ge;
  double acc = 0.0;
  for (int e0 = lane; e0 < sd.n_edges; e0 += 64 * 8) // (same order per lane; eight loads in flight)
  {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
    {
      const int e = e0 + 64 * u;
      v[u] = sd.stats[2 * (e < sd.n_edges ? e : lane) + which];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (e0 + 64 * u < sd.n_edges)
        acc += (double)v[u];
  }
  if (KP && kp.stats && which == 0) // keypoint terms (written by the batched kernel before this one): same slots as the linearize tail
  {
    const float *sk = kp.stats + (photo ? 0 : 2 * (size_t)kp.n_kr);
    const int nk = photo ? kp.n_kr : kp.n_km;
    for (int t = lane; t < nk; t += 64)
      acc += (double)sk[2 * t];
  }
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_down(acc, off);
  if (lane == 0)
  {
    out[which * 2 + (photo ? 0 : 1)] = acc;
    if (mirror)
    {
      // the value, then its ticket: the host spins on the four tickets instead of synchronising the stream
      mirror[which * 2 + (photo ? 0 : 1)] = acc;
      __threadfence_system();
      *reinterpret_cast<volatile double *>(mirror + 4 + which * 2 + (photo ? 0 : 1)) = epoch;
    }
  }
}

__global__ void copy_floats_kernel(const float *__restrict__ src, float *__restrict__ dst, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dst[i] = src[i];
}

// the (reduced) totals -- tail of the packed buffer, error buffer (may be null) -> pinned host mirror.  One wave; the values,
// a workgroup barrier, then one system-scope release and the four tickets in the kernel's OWN slots (mirror[12..15];
// error_totals_kernel owns mirror[8..11]): the host spins on them instead of synchronising the stream
__global__ void mirror_totals_kernel(const double *__restrict__ tail, const double *__restrict__ err,
                                     double *__restrict__ mirror, double epoch)
{
  const int t = threadIdx.x;
  if (t < 4)
    mirror[t] = tail[t];
  else if (t < 8 && err)
    mirror[t] = err[t - 4];
  __syncthreads();
  if (t == 0)
  {
    __threadfence_system();
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<volatile double *>(mirror + 12 + i) = epoch;
  }
}

// dst += src (peer emulation: the contribution of the ranks that are not there)
__global__ void add_doubles_kernel(const double *__restrict__ src, double *__restrict__ dst, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dst[i] += src[i];
}

} // namespace sage
std::vector<int32_t> window_link_pairs(const SageWindow *w)
{
  std::vector<int32_t> lk;
  for (const auto &l : w->links)
    lk.insert(lk.end(), {l.first, l.second});
  return lk;
}

int window_upload_vars(SageWindow *w, int set)
{
  if (w->dpt_set == set)
    w->dpt_set = -1;
  if (set == 0)
    ++w->vars_epoch; // whatever was linearised is no longer the system at the current variables
  std::vector<float> buf((size_t)w->K * w->VS, 0.f);
  for (int k = 0; k < w->K; ++k)
    w->hv.pack(set, k, w->cfg.CS, &buf[(size_t)k * w->VS]);
  SAGE_HIP(hipMemcpyAsync(w->vars[set].p, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream)); // buf is a temporary
  return SAGE_OK;
}


// the batched kernel over this rank's terms at variable set `set`; linearize -> stats_k[0], error pass -> stats_k[1]
static int window_launch_keypoints(SageWindow *w, int set, bool jac)
{
  const int nloc = w->n_kr + w->n_km;
  if (nloc == 0)
    return SAGE_OK;
  KpBatchParams kp{};
  kp.terms = w->kp_table.as<KpTerm>();
  kp.vars = w->vars[set].as<float>();
  kp.VS = w->VS;
  kp.cam = w->cfg.pyr.cam[0];
  kp.eps = w->cfg.eps;
  kp.AtA_r = w->AtA_kr.as<float>(); kp.Atb_r = w->Atb_kr.as<float>();
  kp.AtA_m = w->AtA_km.as<float>(); kp.Atb_m = w->Atb_km.as<float>();
  kp.stats = w->stats_k.as<float>() + (jac ? 0 : (size_t)2 * nloc);
  LaunchCommon lc{};
  prof_attach(w, jac ? 4 : 5, lc);
  if (lc.ev_start)
    (void)hipEventRecord(lc.ev_start, w->stream);
  SAGE_HIP(launch_keypoint_batch(w->stream, w->cfg.CS, jac, nloc, w->n_km > 0, kp));
  if (lc.ev_stop)
    (void)hipEventRecord(lc.ev_stop, w->stream);
  if (jac)
    w->kp_lin = true;
  return SAGE_OK;
}

extern "C" int sage_window_num_keyframes(const SageWindow *w) { return w ? w->K : 0; }
extern "C" int sage_window_num_links(const SageWindow *w) { return w ? (int)w->links.size() : 0; }
extern "C" int sage_window_block_size(const SageWindow *w) { return w ? w->B : 0; }
extern "C" size_t sage_window_packed_count(const SageWindow *w)
{
  if (!w)
    return 0;
  const size_t BB = (size_t)w->B * w->B;
  return (size_t)w->K * BB + w->links.size() * BB + (size_t)w->K * w->B + 4;
}
extern "C" double *sage_window_packed_dev(SageWindow *w) { return w ? w->packed.as<double>() : nullptr; }
extern "C" double *sage_window_error_dev(SageWindow *w) { return w ? w->errbuf.as<double>() : nullptr; }
extern "C" double sage_window_residuals_per_linearize(const SageWindow *w) { return w ? w->residuals_per_lin : 0; }
extern "C" double sage_window_bytes_per_linearize(const SageWindow *w) { return w ? w->bytes_per_lin : 0; }

int window_local_edge(const SageWindow *w, int global_edge)
{
  const auto it = std::lower_bound(w->local_edges.begin(), w->local_edges.end(), global_edge);
  return it != w->local_edges.end() && *it == global_edge ? (int)(it - w->local_edges.begin()) : -1;
}

static LaunchCommon window_lc(SageWindow *w, int type, bool photo_linearize = false)
{
  const DenseSide &sd = w->dense[type];
  LaunchCommon lc{};
  lc.work = sd.work.as<WorkItem>();
  lc.edge_first = sd.first.as<int32_t>();
  lc.edge_tiles = sd.tiles.as<int32_t>();
  lc.n_work = sd.n_work;
  lc.n_edges = w->n_edges;
  lc.partials = sd.part.as<float>();
  lc.tiles_per_block = sd.tpb;
  lc.packed = type == kPhoto;
  if (photo_linearize && w->photo_rec.flush > 0)
  {
    // the linearize (and its per-edge finalize) count partial RECORDS, the error pass work items
    lc.edge_first = w->photo_rec.first.as<int32_t>();
    lc.edge_tiles = w->photo_rec.count.as<int32_t>();
    lc.flush = w->photo_rec.flush;
  }
  return lc;
}

// what the per-edge finalize of either factor type takes from its side (E / P: PhotoEdge / PhotoFinalizeParams, Geo...)
template <class E, class P>
static void finalize_side(P &fp, const DenseSide &sd, int set, const LaunchCommon &lc)
{
  const EdgeOut out = sd.out();
  fp.table = sd.tab[set].as<E>();
  fp.edge_first = lc.edge_first; fp.edge_tiles = lc.edge_tiles; fp.partials = lc.partials;
  fp.AtA = out.AtA; fp.Atb = out.Atb; fp.stats = out.stats; fp.wide = out.wide;
}

static AssembleParams window_assemble_params(SageWindow *w)
{
  const SageWindowConfig &c = w->cfg;
  AssembleParams ap{};
  const bool has = w->n_edges > 0;
  const EdgeOut op = w->dense[kPhoto].out(), og = w->dense[kGeo].out();
  ap.AtA_p = (has && c.use_photo) ? op.AtA : nullptr;
  ap.Atb_p = op.Atb;
  ap.stats_p = (has && c.use_photo) ? op.stats : nullptr;
  ap.wide_p = (has && c.use_photo) ? op.wide : nullptr;
  ap.AtA_g = (has && c.use_geo) ? og.AtA : nullptr;
  ap.Atb_g = og.Atb;
  ap.stats_g = (has && c.use_geo) ? og.stats : nullptr;
  ap.wide_g = (has && c.use_geo) ? og.wide : nullptr;
  ap.adj_start = w->adj_start.as<int32_t>();
  ap.adj = w->adj.as<AdjEntry>();
  ap.links = w->link_edges.as<LinkEdges>();
  ap.packed = w->packed.as<double>();
  ap.tail_mirror = w->kernels_mirror_totals() ? w->mirror.h + TotalsMirror::kTail : nullptr;
  ap.K = w->K;
  ap.nlinks = (int)w->links.size();
  ap.CS = c.CS;
  ap.n_edges_p = w->n_edges;
  ap.n_edges_g = w->n_edges;
  ap.split = 1;
  ap.blocks = nullptr;
  if (w->n_kr + w->n_km > 0)
  {
    ap.AtA_kr = w->AtA_kr.as<float>(); ap.Atb_kr = w->Atb_kr.as<float>();
    ap.AtA_km = w->AtA_km.as<float>(); ap.Atb_km = w->Atb_km.as<float>();
    ap.stats_k = w->stats_k.as<float>();
    ap.link_kp_start = w->kp_link_start.as<int32_t>();
    ap.link_kp = w->kp_link.as<AdjEntry>();
    ap.n_kr = w->n_kr;
    ap.n_km = w->n_km;
  }
  return ap;
}

// linearize every local edge at variable set `set` (0 = current estimate, 1 = candidate) and assemble the packed system
// dst: where the packed system is assembled (default: w->packed); local_blocks: only the blocks this rank's edges touch
// (dst then must hold zeros everywhere else: packed_loc)
// merge: the merged linearize of the two factor types (LaunchCommon::merge_geo_weight) -- the per-edge results are then
// mixed (sage_window_get_edge), the assembled system is the same
int window_linearize_set(SageWindow *w, int set, double *dst, bool local_blocks, bool merge)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  const SageWindowConfig &c = w->cfg;
  const int H = (int)c.pyr.cam[0].h, W = (int)c.pyr.cam[0].w;
  if (w->n_edges > 0)
  {
    // depth maps of every keyframe at the current variables: both factor types read their sample depths from them
    // (an accepted candidate's maps from the error pass are still valid: only the gradients are missing then)
    const bool have_depth = w->dpt_set == set;
    SAGE_HIP(launch_depth_batch(w->stream, c.CS, w->depth_items[set].as<DepthItem>(), w->n_depth, H, W, !have_depth,
                                !(have_depth && w->dgrad_valid)));
    w->dpt_set = set;
    w->dgrad_valid = true;
    // main kernels only (stage 1), then ONE finalize launch for both factor types (window_finalize_kernel)
    LaunchCommon lcg = window_lc(w, kGeo), lcp = window_lc(w, kPhoto, true);
    lcg.stage = 1;
    lcp.stage = 1;
    merge = merge && w->merge_ok;
    lcg.merge_geo_weight = lcp.merge_geo_weight = merge ? c.geo_weight : 0.f;
    if (c.use_geo)
    {
      prof_attach(w, 1, lcg);
      SAGE_HIP(launch_geo_linearize(w->stream, c.CS, nullptr, w->dense[kGeo].tab[set].as<GeoEdge>(), lcg, c.pyr.cam[0], c.eps,
                                    c.geo_loss_param, c.geo_weight, w->dense[kGeo].out()));
    }
    if (c.use_photo)
    {
      prof_attach(w, 0, lcp);
      SAGE_HIP(launch_photo_linearize(w->stream, c.CS, c.FS, nullptr, w->dense[kPhoto].tab[set].as<PhotoEdge>(), lcp, c.pyr,
                                      c.photo_weights, c.eps, w->dense[kPhoto].out()));
    }
    {
      const int rck = window_launch_keypoints(w, set, true); // every keypoint term of this rank: one launch
      if (rck)
        return rck;
    }
    WindowFinalizeParams fp{};
    fp.n_p = c.use_photo ? w->n_edges : 0;
    fp.n_g = c.use_geo ? w->n_edges : 0;
    finalize_side<PhotoEdge>(fp.ph, w->dense[kPhoto], set, lcp);
    for (int l = 0; l < c.pyr.levels; ++l)
      fp.ph.wsum += c.photo_weights[l];
    finalize_side<GeoEdge>(fp.ge, w->dense[kGeo], set, lcg);
    fp.ge.weight = c.geo_weight;
    if (merge)
    {
      fp.ge.photo_partials = lcp.partials;
      fp.ge.photo_rec_first = lcp.edge_first;
      fp.ge.photo_rec_count = lcp.edge_tiles;
    }
    if (c.CS == 32)
      hipLaunchKernelGGL((window_finalize_kernel<32>), dim3(fp.n_p + fp.n_g), dim3(kFinalizeBlock), 0, w->stream, fp);
    else
      hipLaunchKernelGGL((window_finalize_kernel<16>), dim3(fp.n_p + fp.n_g), dim3(kFinalizeBlock), 0, w->stream, fp);
    SAGE_HIP(hipGetLastError());
  }
  AssembleParams ap = window_assemble_params(w);
  if (dst)
    ap.packed = dst;
  // four workgroups of 512 threads per output block: one element per thread (the kernel is a chain of dependent
  // gathers per element -- 17 us; one 1024-thread workgroup per block with two elements per thread took 27 us)
  ap.split = 4;
  int nblocks = w->K + ap.nlinks + 1;
  if (local_blocks && w->dist.n_asm_blocks > 0)
  {
    ap.blocks = w->dist.asm_blocks.as<int32_t>();
    nblocks = w->dist.n_asm_blocks;
  }
  if (w->n_kr + w->n_km > 0)
    hipLaunchKernelGGL(assemble_kernel<true>, dim3(nblocks * ap.split), dim3(512), 0, w->stream, ap);
  else
    hipLaunchKernelGGL(assemble_kernel<false>, dim3(nblocks * ap.split), dim3(512), 0, w->stream, ap);
  SAGE_HIP(hipGetLastError());
  window_phase_mark(w, 1);
  if (ap.packed == w->packed.as<double>()) // (a system assembled elsewhere is booked by the caller)
  {
    w->have_lin = true;
    w->lin_epoch = set == 0 ? w->vars_epoch : 0; // (a candidate's system becomes current only through lm_step's accept)
    w->spec_err_valid = false;
    w->dist.packed_reduced = false;
  }
  return SAGE_OK;
}

extern "C" int sage_window_linearize(SageWindow *w)
{
  if (w)
    window_phase_mark(w, 0); // a caller driving the iteration call by call: it starts here
  return window_linearize_set(w, 0);
}

static int window_error_pass(SageWindow *w, int which, bool speculate_gradients);
extern "C" int sage_window_error(SageWindow *w, int which) { return window_error_pass(w, which, false); }


// speculate_gradients (the LM iteration's candidate evaluation, one GPU): the depth-map gradients of the evaluated set are
// launched right behind the totals -- the stream is idle while the host takes the accept / reject decision, and an accepted
// candidate's next linearize then finds maps AND gradients in place (one launch and 13 us off the accepted iteration; a
// rejected candidate's gradients are never read: the next evaluation rebuilds the maps)
static int window_error_pass(SageWindow *w, int which, bool speculate_gradients)
{
  if (!w || !w->finalized || which < 0 || which > 1)
    return SAGE_E_STATE;
  const SageWindowConfig &c = w->cfg;
  const int H = (int)c.pyr.cam[0].h, W = (int)c.pyr.cam[0].w;
  const bool has = w->n_edges > 0;
  if (has && w->dpt_set != which)
  {
    SAGE_HIP(launch_depth_batch(w->stream, c.CS, w->depth_items[which].as<DepthItem>(), w->n_depth, H, W, true, false));
    w->dpt_set = which;
    w->dgrad_valid = false;
  }
  ErrorTotalsSide ph{}, ge{};
  // both factor types: ONE kernel -- the photometric error kernel also evaluates the geometric edge at the same warp
  // (PhotoEdge::dpt1_geo), which saves the geometric launch (39 us + a gap) of the error pass
  const bool fused = has && c.use_photo && c.use_geo;
  if (has && c.use_photo)
  {
    LaunchCommon lc = window_lc(w, kPhoto);
    prof_attach(w, 2, lc);
    lc.stage = 1; // main kernel only: the per-edge statistics are formed by error_totals_kernel below
    lc.fused_geo_loss_param = fused ? c.geo_loss_param : 0.f;
    SAGE_HIP(launch_photo_error(w->stream, c.CS, c.FS, nullptr, w->dense[kPhoto].tab[which].as<PhotoEdge>(), lc, c.pyr,
                                c.photo_weights, c.eps, w->dense[kPhoto].stats.as<float>()));
    float wsum = 0.f;
    for (int l = 0; l < c.pyr.levels; ++l)
      wsum += c.photo_weights[l];
    ph = ErrorTotalsSide{lc.edge_first, lc.edge_tiles, lc.partials, w->dense[kPhoto].stats.as<float>(), 10.0f * wsum, 1.0f, w->n_edges,
                         fused ? 4 : 2, 0, 1};
    if (fused)
      ge = ErrorTotalsSide{lc.edge_first, lc.edge_tiles, lc.partials, w->dense[kGeo].stats.as<float>(), 10.0f * c.geo_weight,
                           c.geo_weight, w->n_edges, 4, 2, 3};
  }
  if (has && c.use_geo && !fused)
  {
    LaunchCommon lc = window_lc(w, kGeo);
    prof_attach(w, 3, lc);
    lc.stage = 1;
    SAGE_HIP(launch_geo_error(w->stream, c.CS, nullptr, w->dense[kGeo].tab[which].as<GeoEdge>(), lc, c.pyr.cam[0], c.eps,
                              c.geo_loss_param, c.geo_weight, w->dense[kGeo].stats.as<float>()));
    ge = ErrorTotalsSide{lc.edge_first, lc.edge_tiles, lc.partials, w->dense[kGeo].stats.as<float>(), 10.0f * c.geo_weight,
                         c.geo_weight, w->n_edges, 2, 0, 1};
  }
  KpTotals kpt{};
  if (w->n_kr + w->n_km > 0)
  {
    // the terms' errors are summed INSIDE the totals kernel (it overwrites its outputs and posts the mirror tickets)
    const int rck = window_launch_keypoints(w, which, false);
    if (rck)
      return rck;
    kpt = KpTotals{w->stats_k.as<float>() + (size_t)2 * (w->n_kr + w->n_km), w->n_kr, w->n_km};
  }
  w->mirror.err_epoch += 1;
  double *const mirror = w->kernels_mirror_totals() ? w->mirror.h + TotalsMirror::kError : nullptr;
  if (kpt.stats)
    hipLaunchKernelGGL(error_totals_kernel<true>, dim3(1), dim3(1024), 0, w->stream, ph, ge, w->errbuf.as<double>(), mirror,
                       (double)w->mirror.err_epoch, kpt);
  else
    hipLaunchKernelGGL(error_totals_kernel<false>, dim3(1), dim3(1024), 0, w->stream, ph, ge, w->errbuf.as<double>(), mirror,
                       (double)w->mirror.err_epoch, kpt);
  SAGE_HIP(hipGetLastError());
  window_phase_mark(w, 4);
  if (speculate_gradients && has && c.use_geo && w->dpt_set == which && !w->dgrad_valid)
  {
    SAGE_HIP(launch_depth_batch(w->stream, c.CS, w->depth_items[which].as<DepthItem>(), w->n_depth, H, W, false, true));
    w->dgrad_valid = true;
  }
  return SAGE_OK;
}

// After a device solve the candidate variables / delta live in the solver's pinned buffers until the stream has
// drained: refresh the host mirrors (set 1) here.  Returns SAGE_E_NOT_PSD when the factorisation hit a non-positive
// pivot (the candidate is then meaningless).
static int window_total_error(SageWindow *w, int from_linearize, double *err, bool stream_idle);

// Single-rank windows: wait for the error pass by spinning on the tickets its totals kernel writes into the pinned mirror
// (sage_window_error is the last thing in the stream then, and everything enqueued before it has landed too): a host
// thread blocked in hipStreamSynchronize for more than a few dozen microseconds wakes up through an interrupt, 20-30 us
// after the kernel has finished -- on the LM iteration's critical path.  false: no mirror / timed out (the caller
// synchronises the stream as before).
static bool window_spin_totals(SageWindow *w, bool reduced_mirror = false)
{
  // (reduced_mirror: the totals have just been mirrored by mirror_totals_kernel -- its own tickets and epoch)
  if (!w->mirror.h)
    return false;
  if (!reduced_mirror && (!w->kernels_mirror_totals() || w->mirror.err_epoch == 0))
    return false;
  const volatile double *t = w->mirror.h + (reduced_mirror ? TotalsMirror::kMirrorTickets : TotalsMirror::kErrorTickets);
  const double want = (double)(reduced_mirror ? w->mirror.mirror_epoch : w->mirror.err_epoch);
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (!(t[0] == want && t[1] == want && t[2] == want && t[3] == want))
  {
    __builtin_ia32_pause();
    if ((++spins & 0x3ff) == 0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.05)
      return false;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return true;
}

// the window's all-reduce of n doubles + (peer emulation) the absent ranks' share from table entry `iterate`
static int window_allreduce(SageWindow *w, double *buf, size_t n, int iterate)
{
  if (w->dist.allreduce && w->dist.allreduce(buf, n, w->dist.allreduce_user))
    return SAGE_E_STATE;
  if (w->dist.emu_rest && w->dist.emu_n > 0)
  {
    const size_t np = sage_window_packed_count(w);
    const double *rest = w->dist.emu_rest + (size_t)(((iterate % w->dist.emu_n) + w->dist.emu_n) % w->dist.emu_n) * np;
    if (n == np)
      hipLaunchKernelGGL(add_doubles_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, w->stream, rest, buf, np);
    else if (n == 4) // error totals of a candidate: the tail of the absent ranks' system at that iterate
      hipLaunchKernelGGL(add_doubles_kernel, dim3(1), dim3(64), 0, w->stream, rest + np - 4, buf, (size_t)4);
    else
      return SAGE_E_UNSUPPORTED;
    SAGE_HIP(hipGetLastError());
  }
  return SAGE_OK;
}

// out of place: recv = sum over the ranks of send (n = the packed system).  Native RCCL reduces send -> recv directly; a
// plain in-place hook gets a device copy first
__global__ void copy_doubles_kernel(const double *__restrict__ src, double *__restrict__ dst, size_t n);
static int window_allreduce_into(SageWindow *w, const double *send, double *recv, size_t n, int iterate)
{
  if (w->dist.allreduce2)
  {
    if (w->dist.allreduce2(send, recv, n, w->dist.allreduce_user))
      return SAGE_E_STATE;
    SageAllReduceFn keep = w->dist.allreduce;
    w->dist.allreduce = nullptr; // (the sum is done: window_allreduce below only adds the emulated peers' share)
    const int rc = window_allreduce(w, recv, n, iterate);
    w->dist.allreduce = keep;
    return rc;
  }
  hipLaunchKernelGGL(copy_doubles_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, w->stream, send, recv, n);
  SAGE_HIP(hipGetLastError());
  return window_allreduce(w, recv, n, iterate);
}

// enqueue the mirror of the (reduced) totals and their tickets
static int window_mirror_totals(SageWindow *w, bool with_err, const double *system = nullptr)
{
  w->mirror.mirror_epoch += 1;
  hipLaunchKernelGGL(mirror_totals_kernel, dim3(1), dim3(64), 0, w->stream,
                     (system ? system : w->packed.as<double>()) + sage_window_packed_count(w) - 4,
                     with_err ? w->errbuf.as<double>() : nullptr,
                     w->mirror.h, (double)w->mirror.mirror_epoch);
  SAGE_HIP(hipGetLastError());
  return SAGE_OK;
}

int window_sync_candidate(SageWindow *w, bool stream_idle)
{
  if (!w->cand_pending)
    return SAGE_OK;
  if (!stream_idle)
    SAGE_HIP(hipStreamSynchronize(w->stream));
  w->cand_pending = false;
  const DeviceSolver *S = w->solver;
  if (solver_host_status(S) != 0)
    return SAGE_E_NOT_PSD;
  const float *v = solver_host_vars(S);
  for (int k = 0; k < w->K; ++k)
    w->hv.unpack(1, k, w->cfg.CS, v + (size_t)k * w->VS);
  std::memcpy(w->delta.data(), solver_host_delta(S), w->delta.size() * sizeof(double));
  return SAGE_OK;
}

// wait for the totals of the last window_mirror_totals: spin on their tickets (with the kernels of a shard 8x shorter,
// the 20-30 us wake-up of a thread blocked in a stream synchronise would be 4 % of an iteration), take up the candidate
// -- a non-positive pivot of its factorisation shows up there (*not_psd) -- and synchronise only if the spin timed out
static int window_wait_mirror(SageWindow *w, bool *not_psd)
{
  const bool idle = window_spin_totals(w, true);
  const int rc = window_sync_candidate(w, idle);
  if (rc && rc != SAGE_E_NOT_PSD)
    return rc;
  *not_psd = rc == SAGE_E_NOT_PSD;
  if (!idle)
    SAGE_HIP(hipStreamSynchronize(w->stream));
  return SAGE_OK;
}

// prior error terms at a variable set (a9): code prior w*||c||^2/CS per keyframe (code_factor.cpp:99-104, zero
// prior code), scale prior on keyframe 0 w*(ln s0 - ln s)^2 (scale_factor.cpp:102-129), pose prior on kf 0.
static void pose_local(const float *origin, const float *other, double out[6])
{
  // gtsam_traits.h:78-89 : [t1 - R1 R0^T t0, log(R1 R0^T)]
  double Rr[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      Rr[i * 3 + j] = (double)other[i * 3 + 0] * origin[j * 3 + 0] + (double)other[i * 3 + 1] * origin[j * 3 + 1] +
                      (double)other[i * 3 + 2] * origin[j * 3 + 2];
  for (int i = 0; i < 3; ++i)
    out[i] = other[9 + i] - (Rr[i * 3 + 0] * origin[9] + Rr[i * 3 + 1] * origin[10] + Rr[i * 3 + 2] * origin[11]);
  const double tr = Rr[0] + Rr[4] + Rr[8];
  const double cs = std::min(1.0, std::max(-1.0, 0.5 * (tr - 1.0)));
  const double th = std::acos(cs);
  const double k = th < 1e-8 ? 0.5 : th / (2.0 * std::sin(th));
  out[3] = k * (Rr[7] - Rr[5]);
  out[4] = k * (Rr[2] - Rr[6]);
  out[5] = k * (Rr[3] - Rr[1]);
}

// owned_only (sharded windows): the terms of the keyframes THIS rank owns (the other ranks' copies of their variables are
// stale here).  The owned sum takes keyframe 0's scale / pose terms right behind its code term, the full sum behind every
// keyframe's code term: each keeps its order, so neither total moves in the last bit
static double prior_error(const SageWindow *w, int set, bool owned_only = false)
{
  const SageWindowConfig &c = w->cfg;
  double e = 0;
  auto keyframe0_terms = [&] {
    if (c.scale_prior_weight > 0)
    {
      const double d = std::log((double)w->hv.scale_init[0]) - std::log((double)w->hv.scale[set][0]);
      e += c.scale_prior_weight * d * d;
    }
    if (c.pose_prior_weight > 0)
    {
      double loc[6];
      pose_local(&w->hv.pose[set][0], &w->hv.pose_init[0], loc);
      for (int i = 0; i < 6; ++i)
        e += c.pose_prior_weight * loc[i] * loc[i];
    }
  };
  for (int k = 0; k < w->K; ++k)
  {
    if (owned_only && sage_shard_keyframe_owner(w->dist.shard, k) != w->rank)
      continue;
    double s = 0;
    for (int i = 0; i < c.CS; ++i)
      s += (double)w->hv.code[set][(size_t)k * c.CS + i] * w->hv.code[set][(size_t)k * c.CS + i];
    e += c.code_prior_weight * s / c.CS;
    if (owned_only && k == 0)
      keyframe0_terms();
  }
  if (!owned_only)
    keyframe0_terms();
  return e;
}

// total error from the pinned mirror: the edge totals at mirror.h[at], mirror.h[at + 1] (kTail: a system's tail, kError: an error
// pass's totals) plus the prior terms at variable set `set`
static double mirrored_error(const SageWindow *w, int at, int set)
{
  return w->mirror.h[at] + w->mirror.h[at + 1] + prior_error(w, set);
}

extern "C" int sage_window_total_error(SageWindow *w, int from_linearize, double *err)
{
  return window_total_error(w, from_linearize, err, false);
}

// stream_idle: the caller has seen the error pass's tickets (window_spin_totals) -- nothing to synchronise
static int window_total_error(SageWindow *w, int from_linearize, double *err, bool stream_idle)
{
  if (!w || !w->finalized || !err)
    return SAGE_E_STATE;
  double t[4];
  int rcs = window_sync_candidate(w, stream_idle);
  if (rcs && rcs != SAGE_E_NOT_PSD)
    return rcs;
  // a failed factorisation only invalidates the CANDIDATE: the error at the linearisation point is still served
  const int rc_out = from_linearize ? SAGE_OK : rcs;
  if (w->kernels_mirror_totals())
  {
    // the kernels mirrored the totals into pinned host memory (the writers -- ap.tail_mirror, the error_totals mirror -- ask
    // the same predicate; a one-rank RCCL communicator or sage_window_set_allreduce leaves the mirror unwritten and takes
    // the copies below: ADVICE r5)
    if (!stream_idle)
      SAGE_HIP(hipStreamSynchronize(w->stream));
    *err = mirrored_error(w, from_linearize ? TotalsMirror::kTail : TotalsMirror::kError, from_linearize ? 0 : 1);
    return rc_out;
  }
  if (from_linearize)
  {
    const size_t off = sage_window_packed_count(w) - 4;
    SAGE_HIP(hipMemcpyAsync(t, w->packed.as<double>() + off, 4 * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  }
  else
    SAGE_HIP(hipMemcpyAsync(t, w->errbuf.p, 4 * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  *err = t[0] + t[1] + prior_error(w, from_linearize ? 0 : 1);
  return rc_out;
}

// diagonal priors (a9): code prior on every keyframe, scale / pose priors on keyframe 0
static void window_priors(const SageWindow *w, std::vector<double> &dadd, std::vector<double> &gadd)
{
  const SageWindowConfig &c = w->cfg;
  const int K = w->K, B = w->B, CS = c.CS;
  dadd.assign((size_t)K * B, 0.0);
  gadd.assign((size_t)K * B, 0.0);
  for (int k = 0; k < K; ++k)
    for (int i = 0; i < CS; ++i)
    {
      dadd[k * B + 6 + i] += c.code_prior_weight;
      gadd[k * B + 6 + i] += c.code_prior_weight * (0.0 - (double)w->hv.code[0][(size_t)k * CS + i]);
    }
  if (c.scale_prior_weight > 0)
  {
    const double s = w->hv.scale[0][0];
    dadd[6 + CS] += c.scale_prior_weight / (s * s);
    gadd[6 + CS] += c.scale_prior_weight / s * (std::log((double)w->hv.scale_init[0]) - std::log(s));
  }
  if (c.pose_prior_weight > 0)
  {
    double loc[6];
    pose_local(&w->hv.pose[0][0], &w->hv.pose_init[0], loc);
    for (int i = 0; i < 6; ++i)
    {
      dadd[i] += c.pose_prior_weight;
      gadd[i] += c.pose_prior_weight * loc[i];
    }
  }
}

// candidate = retract(current, delta).  local_only (sharded windows): only the keyframes this rank touches, the others
// keep their (stale) current values
static void window_retract_candidate(SageWindow *w, bool local_only)
{
  const int K = w->K, B = w->B, CS = w->cfg.CS;
  if (local_only)
    w->hv.copy_set(1, 0);
  for (int k = 0; k < K; ++k)
  {
    if (local_only && !sage_shard_keyframe_is_local(w->dist.shard, k))
      continue;
    float d6[6];
    for (int i = 0; i < 6; ++i)
      d6[i] = (float)w->delta[(size_t)k * B + i];
    sage_pose_retract(&w->hv.pose[0][(size_t)k * 12], d6, &w->hv.pose[1][(size_t)k * 12]);
    for (int i = 0; i < CS; ++i)
      w->hv.code[1][(size_t)k * CS + i] = w->hv.code[0][(size_t)k * CS + i] + (float)w->delta[(size_t)k * B + 6 + i];
    w->hv.scale[1][k] = w->hv.scale[0][k] + (float)w->delta[(size_t)k * B + 6 + CS];
  }
}

extern "C" int sage_window_solve(SageWindow *w, double damp, double *step_norm)
{
  if (!w || !w->finalized || !w->have_lin)
    return SAGE_E_STATE;
  const SageWindowConfig &c = w->cfg;
  const int K = w->K, B = w->B, CS = c.CS;
  if (w->solver)
  {
    // device path: nothing leaves HBM but the candidate's host mirror (pinned, async); no synchronisation here
    // unless the caller asks for the step norm
    int rc = window_sync_candidate(w); // an unconsumed earlier candidate (a re-solve with another damping)
    if (rc && rc != SAGE_E_NOT_PSD)
      return rc;
    if (w->dpt_set == 1)
      w->dpt_set = -1; // the solve rewrites the candidate set
    rc = solver_run(w->solver, w->stream, w->packed.as<double>(), w->vars[0].as<float>(), w->vars[1].as<float>(), CS,
                    damp, c.code_prior_weight, c.scale_prior_weight, c.pose_prior_weight, w->hv.scale_init[0],
                    &w->hv.pose_init[0]);
    if (rc)
      return rc;
    window_phase_mark(w, 3);
    w->cand_pending = true;
    if (step_norm)
    {
      if ((rc = window_sync_candidate(w)))
        return rc;
      *step_norm = std::sqrt(solver_host_step_norm2(w->solver));
    }
    return SAGE_OK;
  }
  const size_t np = sage_window_packed_count(w);
  static const bool dbg = sage::env_flag("SAGE_DEBUG_TIMING");
  auto tnow = [] { return std::chrono::steady_clock::now(); };
  auto t_a = tnow();
  SAGE_HIP(hipStreamSynchronize(w->stream));
  auto t_b = tnow();
  SAGE_HIP(hipMemcpyAsync(w->host_packed.data(), w->packed.p, np * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  auto t_c = tnow();
  // no device solver: the window has duplicate links (solver_create refused them), the host block solve sums them
  std::vector<double> dadd, gadd;
  window_priors(w, dadd, gadd);
  const std::vector<int32_t> lk = window_link_pairs(w);
  int rcs = sage_block_solve(w->host_packed.data(), K, (int)w->links.size(), lk.data(), B, damp, dadd.data(),
                             gadd.data(), w->delta.data()); // (writes delta only on success)
  if (rcs)
    return rcs;
  auto t_d = tnow();
  double nrm = 0;
  for (double v : w->delta)
    nrm += v * v;
  if (step_norm)
    *step_norm = std::sqrt(nrm);
  window_retract_candidate(w, false);
  const int rcu = window_upload_vars(w, 1);
  if (dbg)
  {
    auto t_e = tnow();
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[sage solve] wait-kernels %.3f d2h %.3f block_solve %.3f retract+h2d %.3f ms\n", ms(t_a, t_b),
            ms(t_b, t_c), ms(t_c, t_d), ms(t_d, t_e));
  }
  return rcu;
}

extern "C" int sage_window_accept(SageWindow *w)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  int rcs = window_sync_candidate(w);
  if (rcs)
    return rcs;
  w->hv.copy_set(0, 1);
  ++w->vars_epoch;
  ++w->dist.emu_cur;
  w->dpt_set = w->dpt_set == 1 ? 0 : -1; // depth maps evaluated at the candidate now belong to the current set
  // (a kernel, not hipMemcpyAsync: a device-to-device copy of 11 KB costs ~10 us of API time on the step's critical path)
  const int nv = w->K * w->VS;
  hipLaunchKernelGGL(copy_floats_kernel, dim3((nv + 255) / 256), dim3(256), 0, w->stream, w->vars[1].as<float>(),
                     w->vars[0].as<float>(), nv);
  SAGE_HIP(hipGetLastError());
  return SAGE_OK;
}

extern "C" int sage_window_reset(SageWindow *w)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  (void)window_sync_candidate(w);
  for (int s = 0; s < 2; ++s)
  {
    w->hv.pose[s] = w->hv.pose_init;
    w->hv.code[s] = w->hv.code_added;
    w->hv.scale[s] = w->hv.scale_init;
  }
  int rc;
  if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
    return rc;
  w->have_lin = false;
  w->dist.emu_cur = 0;
  return SAGE_OK;
}

extern "C" int sage_window_get_keyframe(const SageWindow *w, int kf, float *pose12, float *code, float *scale)
{
  if (!w || kf < 0 || kf >= w->K)
    return SAGE_E_INVALID;
  if (pose12)
    std::memcpy(pose12, &w->hv.pose[0][(size_t)kf * 12], 12 * sizeof(float));
  if (code)
    std::memcpy(code, &w->hv.code[0][(size_t)kf * w->cfg.CS], w->cfg.CS * sizeof(float));
  if (scale)
    *scale = w->hv.scale[0][kf];
  return SAGE_OK;
}

extern "C" int sage_window_set_keyframe(SageWindow *w, int kf, const float *pose12, const float *code, float scale)
{
  if (!w || kf < 0 || kf >= w->K || !pose12 || !code)
    return SAGE_E_INVALID;
  (void)window_sync_candidate(w);
  for (int s = 0; s < 2; ++s)
  {
    std::memcpy(&w->hv.pose[s][(size_t)kf * 12], pose12, 12 * sizeof(float));
    std::memcpy(&w->hv.code[s][(size_t)kf * w->cfg.CS], code, w->cfg.CS * sizeof(float));
    w->hv.scale[s][kf] = scale;
  }
  if (w->finalized)
  {
    int rc;
    if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
      return rc;
  }
  return SAGE_OK;
}

extern "C" int sage_window_get_delta(const SageWindow *w, double *delta)
{
  if (!w || !delta)
    return SAGE_E_INVALID;
  int rcs = window_sync_candidate(const_cast<SageWindow *>(w));
  if (rcs)
    return rcs;
  std::memcpy(delta, w->delta.data(), w->delta.size() * sizeof(double));
  return SAGE_OK;
}

__global__ void add_to_double_kernel(double *p, double v) { p[0] += v; }

// local elimination -> all-reduce of the separator system -> separator solve + back substitution of this rank's
// keyframes -> candidate variables of those keyframes.  *lin_error (optional) receives the total error at the
// linearisation point (edge totals ride in the payload tail, prior terms are contributed by their owners).
// Returns SAGE_E_NOT_PSD consistently on every rank (a rank whose local elimination fails poisons the payload).
static int schur_solve(SageWindow *w, double damp, double *lin_error)
{
  const int K = w->K, B = w->B;
  const size_t np = sage_window_packed_count(w), ns = w->dist.h_sep.size();
  SAGE_HIP(hipMemcpyAsync(w->host_packed.data(), w->packed.p, np * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  std::vector<double> dadd, gadd;
  window_priors(w, dadd, gadd);
  int rc = sage_shard_eliminate(w->dist.shard, w->host_packed.data(), damp, dadd.data(), gadd.data(), w->dist.h_sep.data());
  if (rc && rc != SAGE_E_NOT_PSD)
    return rc;
  if (rc == SAGE_E_NOT_PSD)
  {
    // a failed local elimination is flagged in the spare tail slot [ns-3] (a positive count after the sum: every rank
    // sees it); the separator blocks of this rank are void, the error totals at the linearisation point (tail[0..4],
    // written by sage_shard_eliminate before it factorises) stay finite so that st->error is valid on every rank
    std::fill(w->dist.h_sep.begin(), w->dist.h_sep.end() - 8, 0.0);
    w->dist.h_sep[ns - 3] = 1.0;
  }
  w->dist.h_sep[ns - 4] = prior_error(w, 0, true);
  SAGE_HIP(hipMemcpyAsync(w->dist.sepbuf.p, w->dist.h_sep.data(), ns * sizeof(double), hipMemcpyHostToDevice, w->stream));
  if (w->dist.allreduce(w->dist.sepbuf.as<double>(), ns, w->dist.allreduce_user))
    return SAGE_E_STATE;
  SAGE_HIP(hipMemcpyAsync(w->dist.h_sep.data(), w->dist.sepbuf.p, ns * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  if (lin_error)
    *lin_error = w->dist.h_sep[ns - 8] + w->dist.h_sep[ns - 7] + w->dist.h_sep[ns - 4];
  if (w->dist.h_sep[ns - 3] > 0.0 || std::isnan(w->dist.h_sep[0]))
    return SAGE_E_NOT_PSD;
  w->delta.assign((size_t)K * B, 0.0);
  rc = sage_shard_solve(w->dist.shard, w->dist.h_sep.data(), w->delta.data());
  if (rc)
    return rc; // SAGE_E_NOT_PSD of the separator system: identical on every rank
  window_retract_candidate(w, true);
  w->cand_pending = false;
  return window_upload_vars(w, 1);
}

// after a Schur-mode run every rank holds current variables only for the keyframes it touches: sum the owners' copies
extern "C" int sage_window_sync_variables(SageWindow *w)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  if (!w->dist.shard)
    return SAGE_OK; // every rank solves the whole system: nothing to exchange
  if (!w->dist.allreduce)
    return SAGE_E_STATE;
  const int K = w->K, CS = w->cfg.CS, VS = 13 + CS;
  std::vector<double> buf((size_t)K * VS, 0.0);
  for (int k = 0; k < K; ++k)
    if (sage_shard_keyframe_owner(w->dist.shard, k) == w->rank)
      w->hv.pack(0, k, CS, &buf[(size_t)k * VS]);
  int rc;
  {
    DevBuf d; // the collective's device buffer: gone with this block, on every way out of it
    if ((rc = d.reserve(buf.size() * sizeof(double))))
      return rc;
    SAGE_HIP(hipMemcpyAsync(d.p, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice, w->stream));
    if (w->dist.allreduce(d.as<double>(), buf.size(), w->dist.allreduce_user))
      return SAGE_E_STATE;
    SAGE_HIP(hipMemcpyAsync(buf.data(), d.p, buf.size() * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    SAGE_HIP(hipStreamSynchronize(w->stream));
  }
  for (int s = 0; s < 2; ++s)
    for (int k = 0; k < K; ++k)
      w->hv.unpack(s, k, CS, &buf[(size_t)k * VS]);
  if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
    return rc;
  return SAGE_OK;
}

__global__ void copy_doubles_kernel(const double *__restrict__ src, double *__restrict__ dst, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dst[i] = src[i];
}

// The LM iteration (sage_window_lm_step): one policy -- accept test, give-up test, damping schedule -- around the steps
// of one of three sequences, which take the same decisions and walk the same iterates.  classic: linearize (+ all-reduce
// of `packed`); per evaluation a damped solve and an error pass (+ all-reduce of its 4 totals).  schur (sharded windows
// with a shard plan): linearize; per evaluation a local elimination, an all-reduce of the separator system, the separator
// solve, an error pass and an all-reduce of its 4 totals.  at_candidate: per evaluation a damped solve and a linearize at the
// candidate into packed_save (its finalize kernels deliver the error); accepted: the two buffers swap -- the candidate's
// system IS the next iteration's, nothing is re-evaluated or copied; rejected: `packed` never left.
enum class LmSeq { classic, schur, at_candidate };

// (rank-independent decision: the window's link count, not this rank's share of it -- a rank without links must issue
//  the same collectives as the others).  linearize_at_candidate 0 = automatic: the sequence with one collective and no
//  separate error pass per iteration whenever the window is reduced over ranks (the shard's kernels are short there, the
//  second collective and its host round trip are not), the classic sequence on a single rank
static LmSeq lm_sequence_for(const SageWindow *w, const SageLmConfig *cfg)
{
  const bool sharded = w->dist.allreduce != nullptr; // (a hook on a single-rank window is honoured too)
  if (sharded && w->dist.shard)
    return LmSeq::schur;
  const bool at_candidate = cfg->linearize_at_candidate > 0 || (cfg->linearize_at_candidate == 0 && sharded);
  return at_candidate && !w->links.empty() ? LmSeq::at_candidate : LmSeq::classic;
}

// what one evaluation leaves for a later step of the same iteration
struct LmEval
{
  double cur_tot[4];  // at_candidate: the mirrored totals of the current estimate, put back by a rejection
  bool have_cur_tot;  // (a synchronous non-positive pivot of the solve leaves the mirror alone: nothing to put back)
};

// at_candidate: the (reduced) system at variable set `set` into dst, its totals into the pinned mirror with their tickets
// -- the host never blocks in a stream synchronise on the iteration's critical path.  A reduced window assembles only the
// blocks its own edges touch (into packed_loc) and sums out of place into dst; the emulated peers' share of iterate `it`
// is added behind the sum.  The caller books what dst holds now.
static int window_form_system(SageWindow *w, int set, double *dst, int it)
{
  int rc;
  if (!w->dist.allreduce)
    return (rc = window_linearize_set(w, set, dst, false, true)) ? rc : window_mirror_totals(w, false, dst);
  if ((rc = window_linearize_set(w, set, w->dist.packed_loc.as<double>(), true, true)) ||
      (rc = window_allreduce_into(w, w->dist.packed_loc.as<double>(), dst, sage_window_packed_count(w), it)))
    return rc;
  window_phase_mark(w, 2);
  return window_mirror_totals(w, false, dst);
}

// the system at the current estimate, before the first evaluation (at_candidate: and its error, st->error)
static int lm_prepare(LmSeq seq, SageWindow *w, SageLmState *st)
{
  int rc;
  const bool sharded = w->dist.allreduce != nullptr;
  const size_t np = sage_window_packed_count(w);
  if (seq != LmSeq::at_candidate)
  {
    if ((rc = window_linearize_set(w, 0, nullptr, false, true)) ||
        (seq == LmSeq::classic && sharded && (rc = window_allreduce(w, w->packed.as<double>(), np, w->dist.emu_cur))))
      return rc;
    window_phase_mark(w, 2);
    return SAGE_OK;
  }
  if ((rc = w->packed_save.reserve(np * sizeof(double))))
    return rc;
  if (sharded && !w->dist.packed_loc.p)
  {
    if ((rc = w->dist.packed_loc.reserve(np * sizeof(double))))
      return rc;
    SAGE_HIP(hipMemsetAsync(w->dist.packed_loc.p, 0, np * sizeof(double), w->stream)); // blocks of other ranks: zero for good
  }
  // the system at the current estimate is reused only if it is the GLOBAL one: sage_window_linearize / _prepass and the
  // classic sequence leave a system behind that is not booked as reduced (every rank sees the same flags: same call
  // sequence on all ranks)
  bool mirrored_now = false;
  if (!(w->have_lin && w->lin_epoch == w->vars_epoch && (!sharded || w->dist.packed_reduced)))
  {
    if ((rc = window_form_system(w, 0, w->packed.as<double>(), w->dist.emu_cur)))
      return rc;
    w->have_lin = true;
    w->lin_epoch = w->vars_epoch;
    w->dist.packed_reduced = true; // (summed over the ranks, or nothing to sum)
    w->spec_err_valid = false;
    mirrored_now = true;
  }
  if (!w->spec_err_valid)
  {
    // the totals at the current estimate: mirrored by the evaluation above -- or the system was left by
    // sage_window_linearize (unsharded: mirror its tail now)
    if (!mirrored_now && (rc = window_mirror_totals(w, false)))
      return rc;
    if (!window_spin_totals(w, true))
      SAGE_HIP(hipStreamSynchronize(w->stream));
    w->spec_error = mirrored_error(w, TotalsMirror::kTail, 0);
    w->spec_err_valid = true;
  }
  st->error = w->spec_error;
  return SAGE_OK;
}

// one damped solve at st->damp and the candidate's error -> st->candidate_error (INFINITY for a non-positive pivot,
// reported by the solve at once or by window_sync_candidate: a rejected evaluation, not a hard error -- every rank factors
// the same reduced system, so all of them take that branch together and issue the same collectives).  first: classic and
// schur learn st->error here
static int lm_evaluate(LmSeq seq, SageWindow *w, SageLmState *st, bool first, LmEval &ev)
{
  int rc;
  const bool sharded = w->dist.allreduce != nullptr;
  if (seq == LmSeq::schur)
  {
    double lin_error = 0;
    if ((rc = schur_solve(w, st->damp, &lin_error)) && rc != SAGE_E_NOT_PSD)
      return rc;
    window_phase_mark(w, 3);
    if (first)
      st->error = lin_error;
    st->candidate_error = INFINITY;
    if (rc == SAGE_E_NOT_PSD)
      return SAGE_OK;
    if ((rc = sage_window_error(w, 1)))
      return rc;
    hipLaunchKernelGGL(add_to_double_kernel, dim3(1), dim3(1), 0, w->stream, w->errbuf.as<double>(),
                       prior_error(w, 1, true));
    if (w->dist.allreduce(w->errbuf.as<double>(), 4, w->dist.allreduce_user))
      return SAGE_E_STATE;
    double t4[4];
    SAGE_HIP(hipMemcpyAsync(t4, w->errbuf.p, sizeof(t4), hipMemcpyDeviceToHost, w->stream));
    SAGE_HIP(hipStreamSynchronize(w->stream));
    st->candidate_error = t4[0] + t4[1];
    return SAGE_OK;
  }
  // everything of one evaluation is enqueued before the host looks at a number
  rc = sage_window_solve(w, st->damp, nullptr);
  if (rc == SAGE_E_NOT_PSD) // (no error pass, no collective)
  {
    st->candidate_error = INFINITY;
    return first && seq == LmSeq::classic ? sage_window_total_error(w, 1, &st->error) : SAGE_OK;
  }
  if (rc)
    return rc;
  if (seq == LmSeq::at_candidate)
  {
    std::memcpy(ev.cur_tot, w->mirror.h, sizeof(ev.cur_tot)); // (mirrored and seen at the end of the previous evaluation)
    ev.have_cur_tot = true;
    bool not_psd;
    if ((rc = window_form_system(w, 1, w->packed_save.as<double>(), w->dist.emu_cur + 1)) ||
        (rc = window_wait_mirror(w, &not_psd)))
      return rc;
    st->candidate_error = not_psd ? INFINITY : mirrored_error(w, TotalsMirror::kTail, 1);
    return SAGE_OK;
  }
  if ((rc = window_error_pass(w, 1, !sharded)))
    return rc;
  if (!sharded)
  {
    // the error at the linearisation point (tail of the packed buffer) is read together with the candidate's
    const bool idle = window_spin_totals(w);
    if (first && (rc = window_total_error(w, 1, &st->error, idle)))
      return rc;
    if ((rc = window_total_error(w, 0, &st->candidate_error, idle)) == SAGE_E_NOT_PSD)
      st->candidate_error = INFINITY;
    return rc == SAGE_E_NOT_PSD ? SAGE_OK : rc;
  }
  bool not_psd;
  if ((rc = window_allreduce(w, w->errbuf.as<double>(), 4, w->dist.emu_cur + 1)) || (rc = window_mirror_totals(w, true)) ||
      (rc = window_wait_mirror(w, &not_psd)))
    return rc;
  if (first)
    st->error = mirrored_error(w, TotalsMirror::kTail, 0);
  st->candidate_error = not_psd ? INFINITY : mirrored_error(w, TotalsMirror::kError, 1);
  return SAGE_OK;
}

// the candidate becomes the current estimate (at_candidate: and its system, formed in packed_save, the current system)
static int lm_accept(LmSeq seq, SageWindow *w, const SageLmState *st)
{
  const int rc = sage_window_accept(w);
  if (rc || seq != LmSeq::at_candidate)
    return rc;
  w->packed.swap(w->packed_save);
  w->lin_epoch = w->vars_epoch;
  w->dist.packed_reduced = true; // (summed over the ranks by window_form_system, or nothing to sum)
  w->spec_error = st->candidate_error;
  return SAGE_OK;
}

// the candidate is dropped (at_candidate: the mirror goes back to the current estimate's totals)
static void lm_reject(SageWindow *w, const LmEval &ev)
{
  if (ev.have_cur_tot)
    std::memcpy(w->mirror.h, ev.cur_tot, sizeof(ev.cur_tot));
}

extern "C" int sage_window_lm_step(SageWindow *w, SageLmState *st, const SageLmConfig *cfg)
{
  if (!w || !st || !cfg)
    return SAGE_E_INVALID;
  if (w->world > 1 && !w->dist.allreduce)
    return SAGE_E_STATE;
  const LmSeq seq = lm_sequence_for(w, cfg);
  auto clampd = [&](double d) { return std::min(std::max((double)cfg->min_damp, d), (double)cfg->max_damp); };
  if (st->iters == 0 && st->damp <= 0)
    st->damp = cfg->init_damp;
  window_phase_mark(w, 0);
  int rc = lm_prepare(seq, w, st);
  if (rc)
    return rc;
  st->accepted = 0;
  for (int evals = 1;; ++evals)
  {
    LmEval ev{};
    if ((rc = lm_evaluate(seq, w, st, evals == 1, ev)))
      return rc;
    if (st->candidate_error < st->error)
    {
      st->accepted = 1;
      if ((rc = lm_accept(seq, w, st)))
        return rc;
      st->damp = clampd(st->damp / cfg->damp_dec_factor);
      break;
    }
    lm_reject(w, ev);
    const bool give_up = st->damp >= cfg->max_damp || (cfg->max_inner_evals > 0 && evals >= cfg->max_inner_evals);
    st->damp = clampd(st->damp * cfg->damp_inc_factor);
    if (give_up)
      break;
  }
  st->iters += 1;
  return SAGE_OK;
}

// n LM iterations in one call (the loop a C++ caller writes around sage_window_lm_step; bench.py uses it so that no Python
// runs between the iterations it times).  trace (optional): n x {error, candidate_error, accepted, damp after the step}.
// Stops early on an error code; *done (optional) = iterations completed.
static int window_lm_run(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace, int *done,
                         double *step_seconds)
{
  if (!w || !st || !cfg || n < 0)
    return SAGE_E_INVALID;
  int i = 0, rc = SAGE_OK;
  auto t_prev = std::chrono::steady_clock::now();
  for (; i < n; ++i)
  {
    if ((rc = sage_window_lm_step(w, st, cfg)))
      break;
    if (trace)
    {
      trace[4 * i + 0] = st->error;
      trace[4 * i + 1] = st->candidate_error;
      trace[4 * i + 2] = (double)st->accepted;
      trace[4 * i + 3] = st->damp;
    }
    if (step_seconds)
    {
      const auto t = std::chrono::steady_clock::now();
      step_seconds[i] = std::chrono::duration<double>(t - t_prev).count();
      t_prev = t;
    }
  }
  if (done)
    *done = i;
  return rc;
}

extern "C" int sage_window_lm_run(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace, int *done)
{
  return window_lm_run(w, st, cfg, n, trace, done, nullptr);
}

// the same with the host wall time of every iteration (step_seconds[n]: from the return of the previous iteration -- the
// call's entry for the first -- to this one's; an iteration returns once its accept / reject decision is taken)
extern "C" int sage_window_lm_run_timed(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace,
                                        int *done, double *step_seconds)
{
  return window_lm_run(w, st, cfg, n, trace, done, step_seconds);
}
