// depth_scale.hip -- sage_depth_scale_ratio: Mapper::CorrectDepthScale (mapper.cpp:237-309) and the loop detector's
// df::CorrectDepthScale (mapping_utils.h:797-865), and sage_median_f32: the torch::median of Mapper::InitOneFrame
// (mapper.cpp:181-185).  The reference warps all M valid pixels of keyframe 0 into keyframe 1, samples keyframe 1's depth
// bias (bilinear) and mask (nearest) there with two grid_sample calls, and takes the torch::median of the selected
// z / depth ratios: about fifteen tensor operations, a nonzero() and an .item().  Here one kernel does the per-point
// arithmetic and an exact radix selection finds the median: no sort, nothing of size M crosses PCIe, one ticket wait.
//
//   depth_scale_point_kernel   per point: warp, bilinear tap of the bias, nearest tap of the mask, ratio -> its order-
//   median_keys_kernel         preserving 32-bit key (4 M bytes, written once), the counts, and the histogram of the keys'
//                              top 11 bits.  (median_keys_kernel: the same for n given values.)
//   select_hist_kernel         pass 1, 2: every workgroup scans the histogram of the pass before (2048 bins: cheaper than a
//                              launch of its own), picks the bin that holds the wanted rank, and counts the next digit (11,
//                              then 10 bits) of the keys under the prefix found so far
//   select_finish_kernel       one workgroup: scans the last histogram -- the key is the value, bit for bit -- publishes
//                              the record into pinned memory and leaves the histograms zeroed for the next call
// A workgroup counts in LDS (integer atomics) and adds its non-empty bins to the global histogram (integer atomics):
// sums of integers, the same whatever order they arrive in.  There is no floating-point sum anywhere in the selection,
// so two calls on the same inputs return the same bytes.  No workgroup waits for another inside a kernel: the passes
// are separate launches on the workspace's stream, every loop is bounded by M or by the bin count.
//
// sage_depth_scale_ratio_batch, sage_median_f32_batch: B rows in the same four launches and one ticket.  The bodies of the
// four kernels are device functions of (a row's parameters, workgroup, workgroups of the row); the *_batch_kernel run them
// over a flat list of (row, workgroup) items with the rows' table as a kernel argument, every row with its own keys,
// scratch and pinned record, so row b returns the single call's bytes.  One row takes the single call's kernels.
#include "runtime_internal.h"
#include "sage_device.h"
#include "depth_scale_plan.h"

namespace
{
// (kSelBins, kSelPasses, kSelMaxBlocks, SelState, SelHost, SelScratch: depth_scale_plan.h, shared with the host-only plan)
static_assert(kSelBlock == kBlock, "a row's workgroups are counted on the host");
constexpr uint32_t kSelNoKey = 0xffffffffu; // the image of a NaN's bit pattern: no value that takes part has this key

__host__ __device__ constexpr int sel_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int sel_bins(int pass) { return pass == 2 ? 1024 : 2048; }

struct SelParams
{
  uint32_t *keys; // [n]: kSelNoKey where the point takes no part (not selected, or a NaN)
  SelScratch *scr;
  SelHost *host;
  int n, drop_nan;
};

// order-preserving key of a float: all bits of a negative flipped, the sign bit of the rest (-0 sorts before +0)
__device__ __forceinline__ uint32_t sel_key(float v)
{
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float sel_value(uint32_t k)
{
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ void sel_hist_zero(uint32_t *s_hist)
{
  for (int i = threadIdx.x; i < kSelBins; i += kBlock)
    s_hist[i] = 0u;
  __syncthreads();
}
__device__ __forceinline__ void sel_hist_flush(const uint32_t *s_hist, uint32_t *g_hist, int nbins)
{
  __syncthreads();
  for (int i = threadIdx.x; i < nbins; i += kBlock)
  {
    const uint32_t c = s_hist[i];
    if (c)
      atomicAdd(g_hist + i, c);
  }
}

// the bin of g_hist[nbins] that holds the element of rank `rank` (0-based, in bin order) and its rank within that bin;
// called by the whole workgroup, every thread returns the same pair.  rank >= the histogram's total: (0, 0).
template <int NBINS>
__device__ __forceinline__ void sel_scan(const uint32_t *g_hist, uint32_t rank, uint32_t *s_sum, uint32_t *s_pick, uint32_t &bin,
                                         uint32_t &rest)
{
  constexpr int per = NBINS / kBlock;
  const int tid = threadIdx.x;
  uint32_t c[per], mine = 0u;
#pragma unroll
  for (int j = 0; j < per; ++j)
  {
    c[j] = g_hist[tid * per + j];
    mine += c[j];
  }
  s_sum[tid] = mine;
  if (tid == 0)
  {
    s_pick[0] = 0u;
    s_pick[1] = 0u;
  }
  __syncthreads();
  uint32_t before = 0u;
  for (int t = 0; t < tid; ++t)
    before += s_sum[t];
  if (rank >= before && rank - before < mine) // (one thread at most)
  {
    uint32_t r = rank - before, at = 0u;
    bool found = false;
#pragma unroll
    for (int j = 0; j < per; ++j)
    {
      if (!found && r < c[j])
      {
        found = true;
        at = (uint32_t)j;
      }
      else if (!found)
        r -= c[j];
    }
    s_pick[0] = (uint32_t)(tid * per) + at;
    s_pick[1] = r;
  }
  __syncthreads();
  bin = s_pick[0];
  rest = s_pick[1];
  __syncthreads(); // (s_sum and s_pick may be written again)
}

// the counts of a workgroup's points: wave-uniform sums -> LDS -> one global add per counter
__device__ __forceinline__ void sel_counts_flush(int n_pos, int n_sel, int n_nan, int *s_cnt, int32_t *g_cnt)
{
  if ((threadIdx.x & 63) == 0)
  {
    atomicAdd(s_cnt + 0, n_pos);
    atomicAdd(s_cnt + 1, n_sel);
    atomicAdd(s_cnt + 2, n_nan);
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x])
    atomicAdd(g_cnt + threadIdx.x, s_cnt[threadIdx.x]);
}

struct DsParams
{
  float R[9], t[3]; // by value: the caller's pose is host memory
  const float *dpt0, *homo, *bias1, *mask;
  const int64_t *loc; // or null: dpt0 holds the M gathered depths
  float eps, fx, fy, cx, cy, w, h;
  int W, H, M;
  float *ratios_out;     // [M] or null
  int32_t *selected_out; // [M] or null
};

struct DsPoint
{
  float ratio;
  bool pos, selected;
};

// one point, operation by operation as the reference's fp32 tensor expressions round (no multiply-add contraction)
__device__ __forceinline__ DsPoint ds_point(const DsParams &P, int i)
{
#pragma clang fp contract(off)
  DsPoint o;
  float d0;
  if (P.loc)
  {
    const long long at = P.loc[i]; // (the reference's index() throws on a location outside the map: here it reads nothing)
    d0 = (at >= 0 && at < (long long)P.W * P.H) ? P.dpt0[at] : NAN;
  }
  else
    d0 = P.dpt0[i];
  const float *hp = P.homo + 3 * (size_t)i;
  const float h0 = hp[0], h1 = hp[1], h2 = hp[2];
  float X[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
  {
    const float rh = P.R[3 * r + 0] * h0 + P.R[3 * r + 1] * h1 + P.R[3 * r + 2] * h2;
    X[r] = d0 * rh + P.t[r];
  }
  o.pos = X[2] > P.eps;
  const float x = X[0] / X[2] * P.fx + P.cx;
  const float y = X[1] / X[2] * P.fy + P.cy;
  // the grid coordinate, then grid_sample's own un-normalisation (align_corners = false): not the identity in fp32
  const float gx = (x + 0.5f) * (2.0f / P.w) - 1.0f, gy = (y + 0.5f) * (2.0f / P.h) - 1.0f;
  const float ix = ((gx + 1.0f) * (float)P.W - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)P.H - 1.0f) / 2.0f;
  const float xmax = (float)(P.W - 1), ymax = (float)(P.H - 1);
  // bilinear, zeros: the four taps in the order nw, ne, sw, se; an in-bounds tap is multiplied in whatever its weight (a
  // NaN texel under a zero weight gives NaN, as in torch); a tap outside, or a non-finite coordinate, adds nothing
  const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  const bool x0in = x0 >= 0.0f && x0 <= xmax, x1in = x1 >= 0.0f && x1 <= xmax; // (false for a NaN)
  const bool y0in = y0 >= 0.0f && y0 <= ymax, y1in = y1 >= 0.0f && y1 <= ymax;
  const float wnw = (x1 - ix) * (y1 - iy), wne = (ix - x0) * (y1 - iy), wsw = (x1 - ix) * (iy - y0), wse = (ix - x0) * (iy - y0);
  const int jx0 = x0in ? (int)x0 : 0, jx1 = x1in ? (int)x1 : 0, jy0 = y0in ? (int)y0 : 0, jy1 = y1in ? (int)y1 : 0;
  float D1 = 0.0f;
  if (x0in && y0in)
    D1 = D1 + P.bias1[jy0 * P.W + jx0] * wnw;
  if (x1in && y0in)
    D1 = D1 + P.bias1[jy0 * P.W + jx1] * wne;
  if (x0in && y1in)
    D1 = D1 + P.bias1[jy1 * P.W + jx0] * wsw;
  if (x1in && y1in)
    D1 = D1 + P.bias1[jy1 * P.W + jx1] * wse;
  // nearest, zeros: the tap index rounded half to even
  const float rx = rintf(ix), ry = rintf(iy);
  const bool ok = rx >= 0.0f && rx <= xmax && ry >= 0.0f && ry <= ymax; // (false for a NaN)
  const float m = ok ? P.mask[(int)ry * P.W + (int)rx] : 0.0f;
  const float valid = m * (o.pos ? 1.0f : 0.0f);
  o.selected = valid > 0.5f;
  o.ratio = (X[2] * valid) / D1; // (the multiplication by the mask value stays; x / 0 = inf is a value and sorts last)
  return o;
}

// the bodies of the four kernels: workgroup `blk` of the `nblk` that share a row.  The single calls run them over a grid of
// their own, a batch over its flat list of (row, workgroup) items: a row is the single call's partition
__device__ __forceinline__ void ds_point_body(const DsParams &P, const SelParams &S, int blk, int nblk)
{
  __shared__ uint32_t s_hist[kSelBins];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x;
  if (tid < 4)
    s_cnt[tid] = 0;
  sel_hist_zero(s_hist);
  int n_pos = 0, n_sel = 0, n_nan = 0; // wave-uniform
  for (long long base = (long long)blk * kBlock; base < P.M; base += (long long)nblk * kBlock) // (no int overflow near 2^31)
  {
    const long long i = base + tid;
    const bool live = i < P.M;
    const DsPoint pt = ds_point(P, live ? (int)i : 0);
    const bool pos = live && pt.pos, sel = live && pt.selected, nan = sel && pt.ratio != pt.ratio;
    n_pos += __popcll(__ballot(pos));
    n_sel += __popcll(__ballot(sel));
    n_nan += __popcll(__ballot(nan));
    if (live)
    {
      const uint32_t key = (sel && !nan) ? sel_key(pt.ratio) : kSelNoKey;
      S.keys[i] = key;
      if (key != kSelNoKey)
        atomicAdd(s_hist + (key >> sel_shift(0)), 1u);
      if (P.ratios_out)
        P.ratios_out[i] = pt.ratio;
      if (P.selected_out)
        P.selected_out[i] = pt.selected ? 1 : 0;
    }
  }
  sel_counts_flush(n_pos, n_sel, n_nan, s_cnt, S.scr->cnt);
  sel_hist_flush(s_hist, S.scr->hist[0], sel_bins(0));
}

// values[loc[i]] (or values[i]) -> keys; every value is "selected"
__device__ __forceinline__ void median_keys_body(const float *values, const int64_t *loc, const SelParams &S, int blk, int nblk)
{
  __shared__ uint32_t s_hist[kSelBins];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x;
  if (tid < 4)
    s_cnt[tid] = 0;
  sel_hist_zero(s_hist);
  int n_nan = 0, n_all = 0; // wave-uniform
  for (long long base = (long long)blk * kBlock; base < S.n; base += (long long)nblk * kBlock)
  {
    const long long i = base + tid;
    const bool live = i < S.n;
    const float v = live ? values[loc ? (long long)loc[i] : i] : 0.0f;
    const bool nan = v != v;
    n_all += __popcll(__ballot(live));
    n_nan += __popcll(__ballot(nan));
    if (live)
    {
      const uint32_t key = nan ? kSelNoKey : sel_key(v);
      S.keys[i] = key;
      if (!nan)
        atomicAdd(s_hist + (key >> sel_shift(0)), 1u);
    }
  }
  sel_counts_flush(n_all, n_all, n_nan, s_cnt, S.scr->cnt);
  sel_hist_flush(s_hist, S.scr->hist[0], sel_bins(0));
}

// pass 1 or 2: the bin of the pass before, then the histogram of this pass's digit under the prefix
__device__ __forceinline__ void select_hist_body(const SelParams &S, int pass, int blk, int nblk)
{
  __shared__ uint32_t s_hist[kSelBins];
  __shared__ uint32_t s_sum[kBlock];
  __shared__ uint32_t s_pick[2];
  const int tid = threadIdx.x;
  uint32_t prefix = 0u, rank;
  if (pass == 1)
  {
    const uint32_t n_keys = (uint32_t)(S.scr->cnt[1] - S.scr->cnt[2]);
    rank = n_keys ? (n_keys - 1u) / 2u : 0u; // the LOWER median
  }
  else
  {
    prefix = S.scr->state[0].prefix;
    rank = S.scr->state[0].rank;
  }
  uint32_t bin, rest;
  sel_scan<kSelBins>(S.scr->hist[pass - 1], rank, s_sum, s_pick, bin, rest); // (passes 0 and 1 both have 2048 bins)
  prefix = (prefix << 11) | bin;
  if (blk == 0 && tid == 0)
  {
    S.scr->state[pass - 1].prefix = prefix;
    S.scr->state[pass - 1].rank = rest;
  }
  sel_hist_zero(s_hist);
  const int shift = sel_shift(pass), above = sel_shift(pass - 1);
  const uint32_t digit_mask = (uint32_t)sel_bins(pass) - 1u;
  for (long long i = (long long)blk * kBlock + tid; i < S.n; i += (long long)nblk * kBlock)
  {
    const uint32_t key = S.keys[i];
    if (key != kSelNoKey && (key >> above) == prefix)
      atomicAdd(s_hist + ((key >> shift) & digit_mask), 1u);
  }
  sel_hist_flush(s_hist, S.scr->hist[pass], sel_bins(pass));
}

__device__ __forceinline__ void select_finish_body(const SelParams &S)
{
  __shared__ uint32_t s_sum[kBlock];
  __shared__ uint32_t s_pick[2];
  const int tid = threadIdx.x;
  const int n_pos = S.scr->cnt[0], n_sel = S.scr->cnt[1], n_nan = S.scr->cnt[2];
  const uint32_t prefix = S.scr->state[1].prefix, rank = S.scr->state[1].rank;
  uint32_t bin, rest;
  sel_scan<1024>(S.scr->hist[2], rank, s_sum, s_pick, bin, rest); // (ends with a barrier: every thread has read the scratch)
  if (tid == 0)
  {
    const int n_keys = n_sel - n_nan;
    const bool nan = n_keys <= 0 || (!S.drop_nan && n_nan > 0); // torch::median: NaN with a NaN present, and of nothing
    S.host->value = nan ? NAN : sel_value((prefix << 10) | bin);
    S.host->n_pos = n_pos;
    S.host->n_selected = n_sel;
    S.host->n_nan = n_nan;
    S.host->n_used = S.drop_nan ? n_keys : n_sel;
  }
  uint32_t *z = reinterpret_cast<uint32_t *>(S.scr); // the next call counts from zero
  for (int i = tid; i < (int)(sizeof(SelScratch) / sizeof(uint32_t)); i += kBlock)
    z[i] = 0u;
}

// ---- the single calls' kernels: one row, the grid is its workgroups ----
__global__ __launch_bounds__(kBlock) void depth_scale_point_kernel(const DsParams P, const SelParams S)
{
  ds_point_body(P, S, blockIdx.x, gridDim.x);
}
// values[loc[i]] (or values[i]) -> keys; every value is "selected"
__global__ __launch_bounds__(kBlock) void median_keys_kernel(const float *values, const int64_t *loc, const SelParams S)
{
  median_keys_body(values, loc, S, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(kBlock) void select_hist_kernel(const SelParams S, int pass)
{
  select_hist_body(S, pass, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(kBlock) void select_finish_kernel(const SelParams S) { select_finish_body(S); }

// ---- the batch's kernels: the same bodies over a flat list of (row, workgroup) items ----
// Row b owns workgroups blk0[b] .. blk0[b + 1] - 1 of the grid (sel_blocks(n[b]) of them: the single call's partition), its
// keys lie at keys + key0[b], its scratch and its pinned record are element b of scr and host.  A flat list keeps rows of
// very different sizes from idling the device: a 2-D grid would launch the largest row's workgroups for every row.  The
// table is a kernel argument (0.5 KB; 3.5 KB with the rows of the per-point kernel): it is read with scalar loads.
struct SelBatch
{
  uint32_t *keys;
  SelScratch *scr; // [B]
  SelHost *host;   // [B]
  int drop_nan, B;
  int n[SAGE_DEPTH_SCALE_MAX_BATCH];
  int blk0[SAGE_DEPTH_SCALE_MAX_BATCH + 1]; // (blk0[b] = the grid for b >= B)
  long long key0[SAGE_DEPTH_SCALE_MAX_BATCH];
};

struct DsRow // what differs between the rows of a depth-scale batch
{
  float R[9], t[3];
  const float *dpt0, *homo;
  const int64_t *loc;
  float *ratios_out;
  int32_t *selected_out;
};
struct DsBatch
{
  DsParams shared; // bias, mask, eps, camera; the row's members are filled in from rows[b]
  DsRow rows[SAGE_DEPTH_SCALE_MAX_BATCH];
};
static_assert(sizeof(DsBatch) + sizeof(SelBatch) <= 3840, "the per-point kernel's arguments stay under the 4 KB limit");

// the row of workgroup blk: how many rows start at or before it (branch-free over the whole table)
__device__ __forceinline__ int sel_row_of(const SelBatch &T, int blk)
{
  int b = 0;
#pragma unroll
  for (int r = 1; r < SAGE_DEPTH_SCALE_MAX_BATCH; ++r)
    b += blk >= T.blk0[r] ? 1 : 0;
  return b;
}
__device__ __forceinline__ SelParams sel_row(const SelBatch &T, int b)
{
  SelParams S;
  S.keys = T.keys + T.key0[b];
  S.scr = T.scr + b;
  S.host = T.host + b;
  S.n = T.n[b];
  S.drop_nan = T.drop_nan;
  return S;
}

__global__ __launch_bounds__(kBlock) void depth_scale_point_batch_kernel(const DsBatch G, const SelBatch T)
{
  const int b = sel_row_of(T, blockIdx.x);
  DsParams P = G.shared;
#pragma unroll
  for (int i = 0; i < 9; ++i)
    P.R[i] = G.rows[b].R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    P.t[i] = G.rows[b].t[i];
  P.dpt0 = G.rows[b].dpt0; P.homo = G.rows[b].homo; P.loc = G.rows[b].loc;
  P.ratios_out = G.rows[b].ratios_out; P.selected_out = G.rows[b].selected_out;
  P.M = T.n[b];
  ds_point_body(P, sel_row(T, b), blockIdx.x - T.blk0[b], T.blk0[b + 1] - T.blk0[b]);
}

struct MedianBatch
{
  const float *values[SAGE_DEPTH_SCALE_MAX_BATCH];
  const int64_t *loc[SAGE_DEPTH_SCALE_MAX_BATCH]; // or null
};
__global__ __launch_bounds__(kBlock) void median_keys_batch_kernel(const MedianBatch V, const SelBatch T)
{
  const int b = sel_row_of(T, blockIdx.x);
  median_keys_body(V.values[b], V.loc[b], sel_row(T, b), blockIdx.x - T.blk0[b], T.blk0[b + 1] - T.blk0[b]);
}
__global__ __launch_bounds__(kBlock) void select_hist_batch_kernel(const SelBatch T, int pass)
{
  const int b = sel_row_of(T, blockIdx.x);
  select_hist_body(sel_row(T, b), pass, blockIdx.x - T.blk0[b], T.blk0[b + 1] - T.blk0[b]);
}
// grid: the rows
__global__ __launch_bounds__(kBlock) void select_finish_batch_kernel(const SelBatch T) { select_finish_body(sel_row(T, blockIdx.x)); }

// the workspace's selection buffers for `rows` rows of n_keys keys in all.  While sel_scratch_zero holds, the WHOLE scratch
// allocation is zero (a finish kernel re-zeroes the rows its call counted in); it is zeroed here when the allocation is new
// or a call did not reach its finish kernel
int sel_reserve_rows(SageWorkspace *ws, size_t n_keys, int rows)
{
  int rc;
  const size_t scratch_cap = ws->sel_scratch.cap; // (not the address: a larger block may come back at the old one)
  if ((rc = ws->sel_keys.reserve(n_keys * sizeof(uint32_t))) || (rc = ws->sel_scratch.reserve((size_t)rows * sizeof(SelScratch))) ||
      (rc = ws->sel_host.reserve((size_t)rows * sizeof(SelHost)))) // (every earlier call has been waited for)
    return rc;
  if (ws->sel_scratch.cap != scratch_cap)
    ws->sel_scratch_zero = false;
  if (!ws->sel_scratch_zero) // (a new allocation, or the call before did not reach its finish kernel)
    SAGE_HIP(hipMemsetAsync(ws->sel_scratch.p, 0, ws->sel_scratch.cap, ws->stream));
  ws->sel_scratch_zero = false; // (until this call's finish kernel has run)
  return SAGE_OK;
}
int sel_reserve(SageWorkspace *ws, int n, int drop_nan, SelParams *S)
{
  int rc;
  if ((rc = sel_reserve_rows(ws, (size_t)n, 1)))
    return rc;
  S->keys = ws->sel_keys.as<uint32_t>();
  S->scr = ws->sel_scratch.as<SelScratch>();
  S->host = ws->sel_host.as<SelHost>();
  S->n = n;
  S->drop_nan = drop_nan ? 1 : 0;
  return SAGE_OK;
}
int sel_reserve_batch(SageWorkspace *ws, const SelBatchPlan &plan, int drop_nan, SelBatch *T)
{
  int rc;
  if ((rc = sel_reserve_rows(ws, (size_t)plan.keys, plan.B)))
    return rc;
  T->keys = ws->sel_keys.as<uint32_t>();
  T->scr = ws->sel_scratch.as<SelScratch>();
  T->host = ws->sel_host.as<SelHost>();
  T->drop_nan = drop_nan ? 1 : 0;
  T->B = plan.B;
  for (int b = 0; b < SAGE_DEPTH_SCALE_MAX_BATCH; ++b)
  {
    T->n[b] = plan.n[b];
    T->key0[b] = plan.key0[b];
  }
  for (int b = 0; b <= SAGE_DEPTH_SCALE_MAX_BATCH; ++b)
    T->blk0[b] = b < plan.B ? plan.blk0[b] : plan.workgroups;
  return SAGE_OK;
}

// after the kernel that wrote the keys: the two digit passes, the finish, the ticket
int sel_run(SageWorkspace *ws, const SelParams &S)
{
  const int nb = sel_blocks(S.n);
  hipStream_t s = ws->stream;
  hipLaunchKernelGGL(select_hist_kernel, dim3(nb), dim3(kBlock), 0, s, S, 1);
  hipLaunchKernelGGL(select_hist_kernel, dim3(nb), dim3(kBlock), 0, s, S, 2);
  hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(kBlock), 0, s, S);
  SAGE_HIP(hipGetLastError());
  int rc;
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  ws->sel_scratch_zero = true;
  return SAGE_OK;
}
int sel_run_batch(SageWorkspace *ws, const SelBatchPlan &plan, const SelBatch &T)
{
  hipStream_t s = ws->stream;
  hipLaunchKernelGGL(select_hist_batch_kernel, dim3(plan.workgroups), dim3(kBlock), 0, s, T, 1);
  hipLaunchKernelGGL(select_hist_batch_kernel, dim3(plan.workgroups), dim3(kBlock), 0, s, T, 2);
  hipLaunchKernelGGL(select_finish_batch_kernel, dim3(plan.B), dim3(kBlock), 0, s, T);
  SAGE_HIP(hipGetLastError());
  int rc;
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  ws->sel_scratch_zero = true;
  ws->sel_batch_launches = plan.launches;
  return SAGE_OK;
}

void ds_shared_params(DsParams *P, const SageCamera *cam, const float *bias1_dev, const float *mask_dev, float eps)
{
  P->bias1 = bias1_dev; P->mask = mask_dev;
  P->eps = eps;
  P->fx = cam->fx; P->fy = cam->fy; P->cx = cam->cx; P->cy = cam->cy; P->w = cam->w; P->h = cam->h;
  P->W = (int)cam->w; P->H = (int)cam->h;
}
} // namespace

extern "C" int sage_depth_scale_ratio(SageWorkspace *ws, const float *R10, const float *t10, const float *dpt0_dev,
                                      const int64_t *loc1d0_dev, const float *homo0_dev, int M, const SageCamera *cam,
                                      const float *bias1_dev, const float *mask_dev, float eps, int drop_nan,
                                      float *ratios_out_dev, int32_t *selected_out_dev, SageDepthScaleStats *out)
{
  if (!ws || !R10 || !t10 || !dpt0_dev || !homo0_dev || !cam || !bias1_dev || !mask_dev || !out || M <= 0)
    return SAGE_E_INVALID;
  if (!depth_scale_camera_ok(cam))
    return SAGE_E_INVALID;
  int rc;
  SelParams S;
  if ((rc = sel_reserve(ws, M, drop_nan, &S)))
    return rc;
  DsParams P;
  std::memcpy(P.R, R10, sizeof(P.R));
  std::memcpy(P.t, t10, sizeof(P.t));
  ds_shared_params(&P, cam, bias1_dev, mask_dev, eps);
  P.dpt0 = dpt0_dev; P.homo = homo0_dev; P.loc = loc1d0_dev;
  P.M = M;
  P.ratios_out = ratios_out_dev; P.selected_out = selected_out_dev;
  hipLaunchKernelGGL(depth_scale_point_kernel, dim3(sel_blocks(M)), dim3(kBlock), 0, ws->stream, P, S);
  if ((rc = sel_run(ws, S)))
    return rc;
  const SelHost *h = S.host;
  out->ratio = h->value;
  out->n_points = M;
  out->n_pos_depth = h->n_pos;
  out->n_selected = h->n_selected;
  out->n_nan = h->n_nan;
  out->n_used = h->n_used;
  return SAGE_OK;
}

extern "C" int sage_median_f32(SageWorkspace *ws, const float *values_dev, const int64_t *loc1d_dev, int n, int drop_nan,
                               float *median_host, int *n_used_host, int *n_nan_host)
{
  if (!ws || !values_dev || !median_host || n <= 0)
    return SAGE_E_INVALID;
  int rc;
  SelParams S;
  if ((rc = sel_reserve(ws, n, drop_nan, &S)))
    return rc;
  hipLaunchKernelGGL(median_keys_kernel, dim3(sel_blocks(n)), dim3(kBlock), 0, ws->stream, values_dev, loc1d_dev, S);
  if ((rc = sel_run(ws, S)))
    return rc;
  *median_host = S.host->value;
  if (n_used_host)
    *n_used_host = S.host->n_used;
  if (n_nan_host)
    *n_nan_host = S.host->n_nan;
  return SAGE_OK;
}

extern "C" int sage_depth_scale_ratio_batch(SageWorkspace *ws, const SageDepthScaleRow *rows, int B, const SageCamera *cam,
                                            const float *bias1_dev, const float *mask_dev, float eps, int drop_nan,
                                            SageDepthScaleStats *out)
{
  if (!ws || !rows || !cam || !bias1_dev || !mask_dev || !out || B < 0 || B > SAGE_DEPTH_SCALE_MAX_BATCH)
    return SAGE_E_INVALID;
  if (!depth_scale_camera_ok(cam))
    return SAGE_E_INVALID;
  int32_t M[SAGE_DEPTH_SCALE_MAX_BATCH];
  for (int b = 0; b < B; ++b)
  {
    if (rows[b].M <= 0 || !rows[b].dpt0_dev || !rows[b].homo0_dev)
      return SAGE_E_INVALID;
    M[b] = rows[b].M;
  }
  ws->sel_batch_launches = 0;
  if (B == 0)
    return SAGE_OK;
  if (B == 1) // one row: the single call's kernels (the batch's measure 8 % slower with one row: profiles/depth_scale_batch_bench.txt)
  {
    const SageDepthScaleRow &r = rows[0];
    const int rc1 = sage_depth_scale_ratio(ws, r.R10, r.t10, r.dpt0_dev, r.loc1d0_dev, r.homo0_dev, r.M, cam, bias1_dev, mask_dev, eps,
                                           drop_nan, r.ratios_out_dev, r.selected_out_dev, out);
    if (rc1 == SAGE_OK)
      ws->sel_batch_launches = kSelFixedLaunches;
    return rc1;
  }
  SelBatchPlan plan;
  sel_batch_plan(M, B, &plan);
  int rc;
  SelBatch T;
  if ((rc = sel_reserve_batch(ws, plan, drop_nan, &T)))
    return rc;
  DsBatch G;
  std::memset(&G, 0, sizeof(G));
  ds_shared_params(&G.shared, cam, bias1_dev, mask_dev, eps);
  for (int b = 0; b < B; ++b)
  {
    DsRow &r = G.rows[b];
    std::memcpy(r.R, rows[b].R10, sizeof(r.R));
    std::memcpy(r.t, rows[b].t10, sizeof(r.t));
    r.dpt0 = rows[b].dpt0_dev; r.homo = rows[b].homo0_dev; r.loc = rows[b].loc1d0_dev;
    r.ratios_out = rows[b].ratios_out_dev; r.selected_out = rows[b].selected_out_dev;
  }
  hipLaunchKernelGGL(depth_scale_point_batch_kernel, dim3(plan.workgroups), dim3(kBlock), 0, ws->stream, G, T);
  if ((rc = sel_run_batch(ws, plan, T)))
    return rc;
  for (int b = 0; b < B; ++b)
  {
    const SelHost &h = T.host[b];
    out[b].ratio = h.value;
    out[b].n_points = M[b];
    out[b].n_pos_depth = h.n_pos;
    out[b].n_selected = h.n_selected;
    out[b].n_nan = h.n_nan;
    out[b].n_used = h.n_used;
  }
  return SAGE_OK;
}

extern "C" int sage_median_f32_batch(SageWorkspace *ws, const float *const *values_dev, const int64_t *const *loc1d_dev,
                                     const int32_t *n, int B, int drop_nan, float *median_host, int32_t *n_used_host,
                                     int32_t *n_nan_host)
{
  if (!ws || B < 0 || B > SAGE_DEPTH_SCALE_MAX_BATCH)
    return SAGE_E_INVALID;
  if (B > 0 && (!values_dev || !n || !median_host))
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
    if (!values_dev[b] || n[b] <= 0)
      return SAGE_E_INVALID;
  ws->sel_batch_launches = 0;
  if (B == 0)
    return SAGE_OK;
  if (B == 1) // (as above)
  {
    const int rc1 = sage_median_f32(ws, values_dev[0], loc1d_dev ? loc1d_dev[0] : nullptr, n[0], drop_nan, median_host, n_used_host,
                                    n_nan_host);
    if (rc1 == SAGE_OK)
      ws->sel_batch_launches = kSelFixedLaunches;
    return rc1;
  }
  SelBatchPlan plan;
  sel_batch_plan(n, B, &plan);
  int rc;
  SelBatch T;
  if ((rc = sel_reserve_batch(ws, plan, drop_nan, &T)))
    return rc;
  MedianBatch V;
  std::memset(&V, 0, sizeof(V));
  for (int b = 0; b < B; ++b)
  {
    V.values[b] = values_dev[b];
    V.loc[b] = loc1d_dev ? loc1d_dev[b] : nullptr;
  }
  hipLaunchKernelGGL(median_keys_batch_kernel, dim3(plan.workgroups), dim3(kBlock), 0, ws->stream, V, T);
  if ((rc = sel_run_batch(ws, plan, T)))
    return rc;
  for (int b = 0; b < B; ++b)
  {
    median_host[b] = T.host[b].value;
    if (n_used_host)
      n_used_host[b] = T.host[b].n_used;
    if (n_nan_host)
      n_nan_host[b] = T.host[b].n_nan;
  }
  return SAGE_OK;
}

extern "C" int sage_depth_scale_ratio_batch_launches(const SageWorkspace *ws) { return ws ? ws->sel_batch_launches : 0; }
