// window_eval.hip -- evaluate a finalized window's factors at a variable set: the linearize (dense kernels, the terms' launches
// of window_terms.hip, one per-edge finalize launch, deterministic assembly into the block-sparse packed system) and the error
// pass with its totals kernel.  Everything here enqueues on the window's stream and returns; who waits for the totals is window_reduce.hip.
#include "runtime_internal.h"
#include "finalize_bodies.h"

namespace sage
{

// B-index (0..6+CS: pose 6, code CS, scale) -> column of the per-edge system, or -1 if absent.  type: the column map = the
// group (window_plan.h) -- 0 the photometric edge's, 1 the geometric edge's, 2 poses and scales only [pose0 pose1 scale0 scale1]
__device__ __forceinline__ int edge_col(int type, int role, int bi, int CS)
{
  if (bi < 6)
    return role * 6 + bi;
  if (type == 2)
    return bi == 6 + CS ? 12 + role : -1; // no code row
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

// the terms' share of an error total: `acc` plus, lane-strided in a fixed order, the errors of the stat array's run that rides
// in the slot -- the leading (reprojection) entries in the photometric one, every other entry in the geometric one
__device__ __forceinline__ double add_term_errors(double acc, const TermResults &r, bool photo, int lane)
{
  const float *sk = r.stats + (photo ? 0 : 2 * (size_t)r.n_photo_stats());
  const int nk = photo ? r.n_photo_stats() : r.n_geo_stats();
  for (int t = lane; t < nk; t += 64)
    acc += (double)sk[2 * t];
  return acc;
}

// one workgroup per output block; thread per element; contributions summed in a fixed order (deterministic)
// KP: the window carries terms (AdjEntry::type >= 2, the link lists, their share of the tail); windows without
// them run the instantiation that knows nothing of them
template <bool KP>
__global__ __launch_bounds__(1024) void assemble_kernel(const AssembleParams p)
{
  const int B = 7 + p.CS, BB = B * B;
  const int Dp = TermResults::dim(0, p.CS), Dg = TermResults::dim(1, p.CS);
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
      const int lt = KP ? adj_group(ae.type) : ae.type;
      const bool kp = KP && ae.type >= 2;
      const int D = TermResults::dim(lt, p.CS);
      const float *A = kp ? p.terms.AtA(lt) : (lt == 0 ? p.AtA_p : p.AtA_g);
      const float *b = kp ? p.terms.Atb(lt) : (lt == 0 ? p.Atb_p : p.Atb_g);
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
      if (KP && p.link_terms_start) // the terms on the link's two directions
        for (int a = p.link_terms_start[l]; a < p.link_terms_start[l + 1]; ++a)
        {
          const AdjEntry ae = p.link_terms[a];
          const int lt = adj_group(ae.type), D = TermResults::dim(lt, p.CS);
          const float *A = p.terms.AtA(lt);
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
    if (KP && p.terms.stats && wave < 2)
      acc = add_term_errors(acc, p.terms, photo, lane);
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
// priors: the marginal-prior terms' table and the error pass's tile partials (window_prior.hip; null without local terms): their
// errors ride in the geometric slot, as in the linearize tail
struct PriorErrors
{
  const marg::PriorTermDev *table;
  const double *part;
  int n_terms;
};

template <bool KP>
__global__ __launch_bounds__(1024) void error_totals_kernel(const ErrorTotalsSide ph, const ErrorTotalsSide ge, double *out,
                                                            double *mirror, double epoch, const TermResults terms,
                                                            const PriorErrors priors)
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
  if (KP && terms.stats && which == 0) // (written by the batched kernels before this one): same slots as the linearize tail
    acc = add_term_errors(acc, terms, photo, lane);
  for (int off = 32; off > 0; off >>= 1)
    acc += __shfl_down(acc, off);
  if (lane == 0)
  {
    if (priors.part && which == 0 && !photo)
      acc += marg::prior_error_total(priors.table, priors.n_terms, priors.part);
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

} // namespace sage

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

// sum of the pyramid levels' photometric weights: what an edge without inliers is charged ten times (finalize, error pass)
static float photo_weight_sum(const SageWindowConfig &c)
{
  float wsum = 0.f;
  for (int l = 0; l < c.pyr.levels; ++l)
    wsum += c.photo_weights[l];
  return wsum;
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
  ap.terms = w->terms.results(true); // (all zero without terms)
  ap.link_terms_start = w->terms.link_start.as<int32_t>();
  ap.link_terms = w->terms.link.as<AdjEntry>();
  return ap;
}

// linearize every local edge at variable set `set` (0 = current estimate, 1 = candidate) and assemble the packed system
// dst: where the packed system is assembled (default: w->packed); local_blocks: only the blocks this rank's edges touch
// (dst then must hold zeros everywhere else: packed_loc)
// merge: the merged linearize of the two factor types (LaunchCommon::merge_geo_weight) -- the per-edge results are then
// mixed (sage_window_get_edge), the assembled system is the same
int window_linearize_set(SageWindow *w, int set, double *dst, bool local_blocks, bool merge, bool stale_only)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  const SageWindowConfig &c = w->cfg;
  const int H = (int)c.pyr.cam[0].h, W = (int)c.pyr.cam[0].w;
  // SAGE_RELIN_STALE: the edges this call evaluates, their depth maps rebuilt and their compacted plan on the device; the
  // main kernels take the edge from WorkItem::edge and the partial slot from the block index or the (compacted) record plan
  RelinLaunch rl;
  if (stale_only)
  {
    if (const int rcr = relin_prepare(w, rl))
      return rcr;
    if (rl.nothing)
      return SAGE_OK;
  }
  // a rank -- or a whole window -- whose links all carry keypoint terms only has no dense edge: no depth batch, no dense
  // kernel and no per-edge finalize then (a launch with a zero grid is an error); its terms are linearized all the same.
  // The same holds for a stale-mode call that finds no dense edge stale
  const bool dense = stale_only ? rl.any() : w->n_edges > 0;
  const bool lin_photo = c.use_photo && (!stale_only || rl.n_edges[kPhoto] > 0);
  const bool lin_geo = c.use_geo && (!stale_only || rl.n_edges[kGeo] > 0);
  LaunchCommon lcg{}, lcp{};
  merge = merge && w->merge_ok && !stale_only;
  if (dense)
  {
    if (!stale_only)
    {
      // depth maps of every keyframe at the current variables: both factor types read their sample depths from them
      // (an accepted candidate's maps from the error pass are still valid: only the gradients are missing then)
      const bool have_depth = w->dpt_set == set, have_grad = have_depth && w->dgrad_valid;
      SAGE_HIP(launch_depth_batch(w->stream, c.CS, w->depth_items[set].as<DepthItem>(), w->n_depth, H, W, !have_depth, !have_grad));
      w->dpt_set = set;
      w->dgrad_valid = true;
      relin_stamp_maps(w, set, !have_depth, !have_grad);
      relin_count_all(w, true, !have_depth, !have_grad);
    }
    // main kernels only (stage 1), then ONE finalize launch for both factor types (window_finalize_kernel)
    ++w->dense_serial; // the per-edge AtA are about to be rewritten (sage_window_prepare_factors_device)
    lcg = window_lc(w, kGeo);
    lcp = window_lc(w, kPhoto, true);
    lcg.stage = 1;
    lcp.stage = 1;
    lcg.merge_geo_weight = lcp.merge_geo_weight = merge ? c.geo_weight : 0.f;
    if (stale_only)
    {
      // the sub work lists; the per-edge item / record counts are the full plan's
      lcg.work = rl.work[kGeo]; lcg.edge_first = rl.first[kGeo]; lcg.n_work = rl.n_items[kGeo];
      lcp.work = rl.work[kPhoto]; lcp.edge_first = rl.first[kPhoto]; lcp.n_work = rl.n_items[kPhoto];
    }
    if (lin_geo)
    {
      prof_attach(w, 1, lcg);
      SAGE_HIP(launch_geo_linearize(w->stream, c.CS, nullptr, w->dense[kGeo].tab[set].as<GeoEdge>(), lcg, c.pyr.cam[0], c.eps,
                                    c.geo_loss_param, c.geo_weight, w->dense[kGeo].out()));
    }
    if (lin_photo)
    {
      prof_attach(w, 0, lcp);
      SAGE_HIP(launch_photo_linearize(w->stream, c.CS, c.FS, nullptr, w->dense[kPhoto].tab[set].as<PhotoEdge>(), lcp, c.pyr,
                                      c.photo_weights, c.eps, w->dense[kPhoto].out()));
    }
  }
  if (const int rct = window_launch_terms(w, set, true)) // every keypoint term of this rank: one launch; every graph term: one more
    return rct;
  if (const int rcp = window_launch_prior_eval(w, set, true)) // every marginal-prior term of this rank: one launch
    return rcp;
  if (dense)
  {
    WindowFinalizeParams fp{};
    fp.n_p = !lin_photo ? 0 : (stale_only ? rl.n_edges[kPhoto] : w->n_edges);
    fp.n_g = !lin_geo ? 0 : (stale_only ? rl.n_edges[kGeo] : w->n_edges);
    finalize_side<PhotoEdge>(fp.ph, w->dense[kPhoto], set, lcp);
    fp.ph.wsum = photo_weight_sum(c);
    fp.ph.edge_list = rl.list[kPhoto]; // (null unless stale_only: workgroup j handles edge j)
    finalize_side<GeoEdge>(fp.ge, w->dense[kGeo], set, lcg);
    fp.ge.weight = c.geo_weight;
    fp.ge.edge_list = rl.list[kGeo];
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
  if (ap.terms.stats)
    hipLaunchKernelGGL(assemble_kernel<true>, dim3(nblocks * ap.split), dim3(512), 0, w->stream, ap);
  else
    hipLaunchKernelGGL(assemble_kernel<false>, dim3(nblocks * ap.split), dim3(512), 0, w->stream, ap);
  SAGE_HIP(hipGetLastError());
  if (const int rcp = window_launch_prior_add(w, ap.packed, ap.tail_mirror)) // the priors' Lambda image, Atb rows and errors on top
    return rcp;
  window_phase_mark(w, 1);
  w->results_epoch = set == 0 ? w->vars_epoch : 0; // (the per-edge and per-term results: sage_window_marginalize)
  if (ap.packed == w->packed.as<double>()) // (a system assembled elsewhere is booked by the caller)
  {
    w->have_lin = true;
    w->lin_epoch = set == 0 ? w->vars_epoch : 0; // (a candidate's system becomes current only through lm_step's accept)
    w->spec_err_valid = false;
    w->dist.packed_reduced = false;
    w->dogleg.solved0 = w->dogleg.products = false; // (a new system: its Gauss-Newton point is yet to be solved for)
  }
  if (stale_only)
    relin_commit(w, rl);
  else
  {
    if (!dense)
      relin_count_all(w, false, false, false);
    w->relin.drop(); // a merged linearize, one at the candidate, one assembled elsewhere: not what the snapshot stands for
  }
  return SAGE_OK;
}

extern "C" int sage_window_linearize(SageWindow *w)
{
  if (w)
    window_phase_mark(w, 0); // a caller driving the iteration call by call: it starts here
  return window_linearize_set(w, 0, nullptr, false, false, w && w->relin.mode == SAGE_RELIN_STALE);
}

// a workgroup's partial record as the totals kernel reads it: floats per record, slot of the error sum, slot of the inlier count
struct PartialRecord
{
  int stride, err_slot, cnt_slot;
};
constexpr PartialRecord kOwnRecord{2, 0, 1};                         // an error kernel of one factor type: {error, inliers}
constexpr PartialRecord kFusedPhoto{4, 0, 1}, kFusedGeo{4, 2, 3};    // the fused one: {photo error, inliers, geo error, inliers}

// one factor type's side of the totals kernel: the work list of the launch that wrote the partials, where its per-edge
// statistics go, the error of an edge without inliers and the scale of the others
static ErrorTotalsSide error_totals_side(const LaunchCommon &lc, float *stats, float fallback, float scale, int n_edges,
                                         PartialRecord rec)
{
  ErrorTotalsSide sd{};
  sd.edge_first = lc.edge_first; sd.edge_tiles = lc.edge_tiles; sd.partials = lc.partials;
  sd.stats = stats;
  sd.fallback = fallback; sd.scale = scale;
  sd.n_edges = n_edges;
  sd.stride = rec.stride; sd.err_off = rec.err_slot; sd.cnt_off = rec.cnt_slot;
  return sd;
}

// speculate_gradients (the LM iteration's candidate evaluation, one GPU): the depth-map gradients of the evaluated set are
// launched right behind the totals -- the stream is idle while the host takes the accept / reject decision, and an accepted
// candidate's next linearize then finds maps AND gradients in place (one launch and 13 us off the accepted iteration; a
// rejected candidate's gradients are never read: the next evaluation rebuilds the maps)
int window_error_pass(SageWindow *w, int which, bool speculate_gradients)
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
    relin_stamp_maps(w, which, true, false);
  }
  // (the per-edge statistics of this pass: the error half of DenseSide::stats -- the linearization's stay)
  float *const stats_p = w->dense[kPhoto].error_stats(), *const stats_g = w->dense[kGeo].error_stats();
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
                                c.photo_weights, c.eps, stats_p));
    ph = error_totals_side(lc, stats_p, 10.0f * photo_weight_sum(c), 1.0f, w->n_edges,
                           fused ? kFusedPhoto : kOwnRecord);
    if (fused)
      ge = error_totals_side(lc, stats_g, 10.0f * c.geo_weight, c.geo_weight, w->n_edges, kFusedGeo);
  }
  if (has && c.use_geo && !fused)
  {
    LaunchCommon lc = window_lc(w, kGeo);
    prof_attach(w, 3, lc);
    lc.stage = 1;
    SAGE_HIP(launch_geo_error(w->stream, c.CS, nullptr, w->dense[kGeo].tab[which].as<GeoEdge>(), lc, c.pyr.cam[0], c.eps,
                              c.geo_loss_param, c.geo_weight, stats_g));
    ge = error_totals_side(lc, stats_g, 10.0f * c.geo_weight, c.geo_weight, w->n_edges, kOwnRecord);
  }
  // the terms' errors are summed INSIDE the totals kernel (it overwrites its outputs and posts the mirror tickets)
  if (const int rct = window_launch_terms(w, which, false))
    return rct;
  if (const int rcp = window_launch_prior_eval(w, which, false)) // ... and so are the marginal priors', from their tile partials
    return rcp;
  PriorErrors pri{};
  pri.part = window_prior_partials(w, false, &pri.n_terms);
  pri.table = w->priors.table.as<marg::PriorTermDev>();
  const TermResults kpt = w->terms.results(false);
  w->mirror.err_epoch += 1;
  double *const mirror = w->kernels_mirror_totals() ? w->mirror.h + TotalsMirror::kError : nullptr;
  if (kpt.stats)
    hipLaunchKernelGGL(error_totals_kernel<true>, dim3(1), dim3(1024), 0, w->stream, ph, ge, w->errbuf.as<double>(), mirror,
                       (double)w->mirror.err_epoch, kpt, pri);
  else
    hipLaunchKernelGGL(error_totals_kernel<false>, dim3(1), dim3(1024), 0, w->stream, ph, ge, w->errbuf.as<double>(), mirror,
                       (double)w->mirror.err_epoch, kpt, pri);
  SAGE_HIP(hipGetLastError());
  window_phase_mark(w, 4);
  if (speculate_gradients && has && c.use_geo && w->dpt_set == which && !w->dgrad_valid)
  {
    SAGE_HIP(launch_depth_batch(w->stream, c.CS, w->depth_items[which].as<DepthItem>(), w->n_depth, H, W, false, true));
    w->dgrad_valid = true;
    relin_stamp_maps(w, which, false, true);
  }
  return SAGE_OK;
}

extern "C" int sage_window_error(SageWindow *w, int which) { return window_error_pass(w, which, false); }
