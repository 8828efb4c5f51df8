// overlap.hip -- sage_track_overlap: CameraTracker::ComputeAreaInlierRatio (camera_tracker.cpp:95-169) over all M valid
// pixels of the keyframe.  The reference samples the mask with a torch grid_sample, copies both point sets (M x 2 floats
// each) to the host and runs two O(M log M) convex hulls there, per tracked frame.  Here the device does the per-point
// arithmetic, the sums, and an Akl-Toussaint filter: the points strictly inside a polygon of kOvDirs extreme points of
// their set cannot be hull vertices and stay on the device; the few that remain go to the host hull
// (sage_convex_hull_area) through pinned memory.  ~1 MB of input at M = 58 000: the cost is launches and what crosses
// PCIe, so there are three small launches and the ticket, no copy and no stream synchronise.
//
//   overlap_reduce_kernel   per point: warp, projection, mask tap; per workgroup: |pos|, |in|, the motion sum (double) and
//                           the extreme point of each set in kOvDirs directions -> one partial record per workgroup
//   overlap_filter_kernel   every workgroup folds the records' extremes into the two polygons (small: saves a launch),
//                           recomputes its points (cheaper than storing 2 * M * 8 bytes) and appends those not strictly
//                           inside the polygon of their set (wave-aggregated counter)
//   overlap_finish_kernel   one workgroup: totals in workgroup order, header and survivors -> pinned memory
// Sums run over per-workgroup partials in a fixed order and the host hull sorts its input: two calls on the same inputs
// return the same bytes, whatever order the appends arrive in.
//
// sage_track_overlap_batch: B poses over ONE point set, camera and mask (the loop detector's tracked candidates).  The same
// three launches with the pose on blockIdx.y; a row is the single call's partition and the single call's bodies, so row b
// returns the single call's bytes.  The input set does not depend on the pose: row 0's workgroups reduce, filter and
// append it (they are the single call as it is), the other rows carry the warped set alone, and the finish kernel runs
// one workgroup per set (B + 1).  The host hulls the input set once: B + 1 hulls, one wait.
#include "runtime_internal.h"
#include "sage_device.h"

#include <utility>

namespace
{
constexpr int kOvDirs = 16;            // directions of the extreme-point polygon: an ellipse keeps ~2.5 % of its points (8: ~10 %)
constexpr int kOvSlots = 2 * kOvDirs;  // (set, direction); set 0 = the input points (x0, y0), set 1 = the warped in-mask points
constexpr int kOvMaxBlocks = 32;       // workgroups of the two passes; the rest of the points is grid-strided
// a point is dropped when every edge's cross product exceeds kOvMargin * (|e.x * d.y| + |e.y * d.x|): the fp32 evaluation
// of the cross product is off by at most ~4 * 2^-24 of that sum, so a point on or outside an edge is always kept
constexpr float kOvMargin = 1.0e-5f;

// unit vectors at k * 360 / kOvDirs degrees
__device__ const float kOvCos[kOvDirs] = {1.f, 0.92387953f, 0.70710678f, 0.38268343f, 0.f, -0.38268343f, -0.70710678f, -0.92387953f,
                                          -1.f, -0.92387953f, -0.70710678f, -0.38268343f, 0.f, 0.38268343f, 0.70710678f, 0.92387953f};
__device__ const float kOvSin[kOvDirs] = {0.f, 0.38268343f, 0.70710678f, 0.92387953f, 1.f, 0.92387953f, 0.70710678f, 0.38268343f,
                                          0.f, -0.38268343f, -0.70710678f, -0.92387953f, -1.f, -0.92387953f, -0.70710678f, -0.38268343f};

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the per-lane extremes are indexed by compile-time
// constants only, from the source on -- a loop, even one that is unrolled later, has the arrays promoted to 32-wide vector
// registers first and every conditional update copies them whole
template <class F, int... K>
__device__ __forceinline__ void ov_unrolled(F &&f, std::integer_sequence<int, K...>)
{
  (f(std::integral_constant<int, K>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void ov_for(F &&f)
{
  ov_unrolled(f, std::make_integer_sequence<int, N>{});
}

struct OvHeader // head of the pinned region
{
  int32_t n_pos, n_in, n_cand[2];
  double motion_sum;
  double pad;
};

struct OvParams
{
  float R[9], t[3]; // by value: the caller's pose is host memory
  const float *dpts0, *homo, *mask;
  float depth_scale, eps;
  float fx, fy, cx, cy, w, h;
  int W, H, M;
  // partial records, one per workgroup of the reduce pass
  double *part_motion;  // [nb]
  int32_t *part_count;  // [nb][2]: |pos|, |in|
  float *part_ext;      // [nb][kOvSlots][3]: projection, x, y (projection -inf: the set is empty)
  int32_t *n_surv[2];   // append counter of each set
  float *surv[2];       // [M][2] each
  OvHeader *host_head;  // pinned
  float *host_surv[2];  // pinned, [M][2] each
};

struct OvPoint
{
  float x0, y0, x1, y1;
  bool pos, in;
};

// one point, operation by operation as the reference's fp32 tensor expressions round (no multiply-add contraction)
__device__ __forceinline__ OvPoint ov_point(const OvParams &P, int i)
{
#pragma clang fp contract(off)
  OvPoint o;
  const float sd = P.depth_scale * P.dpts0[i];
  const float h0 = P.homo[3 * i + 0], h1 = P.homo[3 * i + 1], h2 = P.homo[3 * i + 2];
  float X[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
  {
    const float rh = P.R[3 * r + 0] * h0 + P.R[3 * r + 1] * h1 + P.R[3 * r + 2] * h2;
    X[r] = sd * rh + P.t[r];
  }
  o.pos = X[2] > P.eps;
  o.x1 = X[0] / X[2] * P.fx + P.cx;
  o.y1 = X[1] / X[2] * P.fy + P.cy;
  o.x0 = h0 * P.fx + P.cx;
  o.y0 = h1 * P.fy + P.cy;
  // grid_sample(nearest, zeros, align_corners = true) at 2 * x / w - 1: the tap index, rounded half to even
  const float gx = 2.0f * o.x1 / P.w - 1.0f, gy = 2.0f * o.y1 / P.h - 1.0f;
  const float rx = rintf((gx + 1.0f) / 2.0f * (P.w - 1.0f)), ry = rintf((gy + 1.0f) / 2.0f * (P.h - 1.0f));
  const bool ok = rx >= 0.0f && rx <= (float)(P.W - 1) && ry >= 0.0f && ry <= (float)(P.H - 1); // (false for a NaN)
  const int ix = ok ? (int)rx : 0, iy = ok ? (int)ry : 0;
  const float m = ok ? P.mask[iy * P.W + ix] : 0.0f;
  o.in = o.pos && m > 0.5f;
  return o;
}

// the reduce pass of one workgroup: partial record `blk` of P's row.  kInput: the input set's extremes as well (slots
// 0..kOvDirs-1 and its append counter); without it the row carries the warped set alone and those slots are not touched
template <bool kInput>
__device__ __forceinline__ void ov_reduce_body(const OvParams &P, int blk, int nblk)
{
  __shared__ float s_ext[kWaves][kOvSlots][3];
  __shared__ double s_motion[kWaves];
  __shared__ int s_count[kWaves][2];
  constexpr int kFirst = kInput ? 0 : kOvDirs; // first slot of the record this row owns
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float bp[kOvSlots], bx[kOvSlots], by[kOvSlots];
  ov_for<kOvSlots>([&](auto s) {
    bp[s()] = -INFINITY;
    bx[s()] = 0.f;
    by[s()] = 0.f;
  });
  double motion = 0.0;
  int n_pos = 0, n_in = 0; // wave-uniform
  for (int base = blk * kBlock; base < P.M; base += nblk * kBlock)
  {
    const bool valid = base + tid < P.M;
    const OvPoint pt = ov_point(P, valid ? base + tid : 0);
    const bool pos = valid && pt.pos, in = valid && pt.in;
    n_pos += __popcll(__ballot(pos));
    n_in += __popcll(__ballot(in));
    if (pos)
    {
      const float dx = pt.x1 - pt.x0, dy = pt.y1 - pt.y0;
      motion += (double)sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))); // the norm in fp32, the sum in double
    }
    ov_for<kOvDirs>([&](auto kc) {
      constexpr int k = kc();
      if constexpr (kInput)
      {
        const float p0 = kOvCos[k] * pt.x0 + kOvSin[k] * pt.y0;
        const bool up0 = valid && p0 > bp[k];
        bp[k] = up0 ? p0 : bp[k];
        bx[k] = up0 ? pt.x0 : bx[k];
        by[k] = up0 ? pt.y0 : by[k];
      }
      const float p1 = kOvCos[k] * pt.x1 + kOvSin[k] * pt.y1;
      const bool up1 = in && p1 > bp[kOvDirs + k];
      bp[kOvDirs + k] = up1 ? p1 : bp[kOvDirs + k];
      bx[kOvDirs + k] = up1 ? pt.x1 : bx[kOvDirs + k];
      by[kOvDirs + k] = up1 ? pt.y1 : by[kOvDirs + k];
    });
  }
  // wave level: the largest projection, then the (x, y) of the first lane that holds it -- the triple travels together
  ov_for<kOvSlots>([&](auto sc) {
    constexpr int s = sc();
    if constexpr (s >= kFirst)
    {
      float m = bp[s];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
        m = fmaxf(m, __shfl_xor(m, off));
      const unsigned long long holders = __ballot(bp[s] == m);
      const int src = holders ? __ffsll((long long)holders) - 1 : 0;
      const float x = __shfl(bx[s], src), y = __shfl(by[s], src);
      if (lane == 0)
      {
        s_ext[wave][s][0] = m;
        s_ext[wave][s][1] = x;
        s_ext[wave][s][2] = y;
      }
    }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) // (a butterfly: every lane ends with the same sum, in the same order every run)
    motion += __shfl_xor(motion, off);
  if (lane == 0)
  {
    s_motion[wave] = motion;
    s_count[wave][0] = n_pos;
    s_count[wave][1] = n_in;
  }
  __syncthreads();
  // through LDS: the waves in order, the first of equal projections wins
  if (tid >= kFirst && tid < kOvSlots)
  {
    int best = 0;
    for (int wv = 1; wv < kWaves; ++wv)
      if (s_ext[wv][tid][0] > s_ext[best][tid][0])
        best = wv;
    float *dst = P.part_ext + ((size_t)blk * kOvSlots + tid) * 3;
    dst[0] = s_ext[best][tid][0];
    dst[1] = s_ext[best][tid][1];
    dst[2] = s_ext[best][tid][2];
  }
  if (tid == 0)
  {
    double ms = 0.0;
    int c0 = 0, c1 = 0;
    for (int wv = 0; wv < kWaves; ++wv)
    {
      ms += s_motion[wv];
      c0 += s_count[wv][0];
      c1 += s_count[wv][1];
    }
    P.part_motion[blk] = ms;
    P.part_count[2 * blk + 0] = c0;
    P.part_count[2 * blk + 1] = c1;
    if (blk == 0) // the filter pass appends from zero (it starts after this kernel has ended)
    {
      if constexpr (kInput)
        *P.n_surv[0] = 0;
      *P.n_surv[1] = 0;
    }
  }
}

__global__ __launch_bounds__(kBlock) void overlap_reduce_kernel(const OvParams P)
{
  ov_reduce_body<true>(P, blockIdx.x, gridDim.x);
}

// strictly inside the polygon s_v[0..nv): left of every edge by more than the margin.  A closed chain that a point sees
// counter-clockwise edge by edge winds around it, so the point lies strictly inside the hull of the chain's corners, which
// are points of the set: it is no hull vertex, whatever shape rounding gave the chain.  nv == 0: no polygon, nothing inside.
__device__ __forceinline__ bool ov_inside(const float (*s_v)[2], int nv, float px, float py)
{
  bool inside = nv > 0;
  for (int j = 0; j < nv; ++j)
  {
    const int jn = j + 1 < nv ? j + 1 : 0;
    const float ax = s_v[j][0], ay = s_v[j][1];
    const float ex = s_v[jn][0] - ax, ey = s_v[jn][1] - ay;
    const float dx = px - ax, dy = py - ay;
    const float t1 = ex * dy, t2 = ey * dx;
    inside = inside && (t1 - t2 > kOvMargin * (fabsf(t1) + fabsf(t2))); // (false for a NaN: kept)
  }
  return inside;
}

// append the lanes' points with one counter add per wave; called by all 64 lanes
__device__ __forceinline__ void ov_append(bool keep, float x, float y, int32_t *counter, float *dst, int cap, int lane)
{
  const unsigned long long b = __ballot(keep);
  if (b == 0)
    return;
  int base = 0;
  if (lane == 0)
    base = atomicAdd(counter, (int)__popcll(b));
  base = __shfl(base, 0);
  const int at = base + (int)__popcll(b & ((1ull << lane) - 1ull));
  if (keep && at < cap) // (every point is appended at most once: at < M always; the check keeps the store in bounds regardless)
  {
    dst[2 * at + 0] = x;
    dst[2 * at + 1] = y;
  }
}

// the filter pass of one workgroup of P's row: fold the row's nb records into the polygon of each set the row owns (kInput:
// both; otherwise the warped set alone), then append the points that are not strictly inside
template <bool kInput>
__device__ __forceinline__ void ov_filter_body(const OvParams &P, int blk, int nblk, int nb)
{
  __shared__ float s_raw[kOvSlots][3];
  __shared__ float s_v[2][kOvDirs][2];
  __shared__ int s_nv[2];
  constexpr int kFirst = kInput ? 0 : kOvDirs, kFirstSet = kInput ? 0 : 1;
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid >= kFirst && tid < kOvSlots) // the records in workgroup order, the first of equal projections wins
  {
    const float *src = P.part_ext + (size_t)tid * 3;
    float m = src[0], x = src[1], y = src[2];
    for (int b = 1; b < nb; ++b)
    {
      const float *q = src + (size_t)b * kOvSlots * 3;
      if (q[0] > m)
      {
        m = q[0];
        x = q[1];
        y = q[2];
      }
    }
    s_raw[tid][0] = m;
    s_raw[tid][1] = x;
    s_raw[tid][2] = y;
  }
  __syncthreads();
  if (tid >= kFirstSet && tid < 2) // the polygon of set `tid`: its extremes by direction, repeated corners (degenerate edges) skipped
  {
    int n = 0;
    for (int k = 0; k < kOvDirs; ++k)
    {
      const float *e = s_raw[tid * kOvDirs + k];
      if (!(e[0] > -INFINITY)) // (empty set)
        continue;
      if (n > 0 && e[1] == s_v[tid][n - 1][0] && e[2] == s_v[tid][n - 1][1])
        continue;
      s_v[tid][n][0] = e[1];
      s_v[tid][n][1] = e[2];
      ++n;
    }
    if (n > 1 && s_v[tid][n - 1][0] == s_v[tid][0][0] && s_v[tid][n - 1][1] == s_v[tid][0][1])
      --n;
    s_nv[tid] = n >= 3 ? n : 0;
  }
  __syncthreads();
  const int nv0 = kInput ? s_nv[0] : 0, nv1 = s_nv[1];
  for (int base = blk * kBlock; base < P.M; base += nblk * kBlock)
  {
    const bool valid = base + tid < P.M;
    const OvPoint pt = ov_point(P, valid ? base + tid : 0);
    if constexpr (kInput)
    {
      const bool keep0 = valid && !ov_inside(s_v[0], nv0, pt.x0, pt.y0);
      ov_append(keep0, pt.x0, pt.y0, P.n_surv[0], P.surv[0], P.M, lane);
    }
    const bool keep1 = valid && pt.in && !ov_inside(s_v[1], nv1, pt.x1, pt.y1);
    ov_append(keep1, pt.x1, pt.y1, P.n_surv[1], P.surv[1], P.M, lane);
  }
}

__global__ __launch_bounds__(kBlock) void overlap_filter_kernel(const OvParams P, int nb)
{
  ov_filter_body<true>(P, blockIdx.x, gridDim.x, nb);
}

// one lane: the totals of P's row in workgroup order -> its header
__device__ __forceinline__ void ov_totals(const OvParams &P, int nb)
{
  double ms = 0.0;
  int n_pos = 0, n_in = 0;
  for (int b = 0; b < nb; ++b) // workgroup order
  {
    ms += P.part_motion[b];
    n_pos += P.part_count[2 * b + 0];
    n_in += P.part_count[2 * b + 1];
  }
  P.host_head->n_pos = n_pos;
  P.host_head->n_in = n_in;
  P.host_head->motion_sum = ms;
}

// one workgroup: set `set` of P's row -> its pinned region; returns how many points that is
__device__ __forceinline__ int ov_publish(const OvParams &P, int set, int tid)
{
  const int c = min(*P.n_surv[set], P.M);
  for (int i = tid; i < 2 * c; i += kBlock)
    P.host_surv[set][i] = P.surv[set][i];
  return c;
}

__global__ __launch_bounds__(kBlock) void overlap_finish_kernel(const OvParams P, int nb)
{
  const int tid = threadIdx.x;
  const int c0 = ov_publish(P, 0, tid), c1 = ov_publish(P, 1, tid);
  if (tid == 0)
  {
    ov_totals(P, nb);
    P.host_head->n_cand[0] = c0;
    P.host_head->n_cand[1] = c1;
  }
}

// The workspace's three regions, by row.  A row is one pose: its partial records and append counters in ov_part, its warped
// set's survivors in ov_surv and in the pinned region, its header.  The input set (set 0) is row 0's: every row's n_surv[0],
// surv[0] and host_surv[0] name the same memory.  The single call is this layout with B = 1.
//   ov_part  [row][motion double kOvMaxBlocks | counts int32 2 kOvMaxBlocks | append counters int32 2 (+ 2 pad) |
//                  extremes float kOvMaxBlocks * slots * 3]
//   ov_surv  [input set [M][2] | warped set of row b [M][2], b < B]
//   ov_host  [header [B] | input set [M][2] | warped set of row b [M][2], b < B]
constexpr size_t kOvPartBytes = kOvMaxBlocks * sizeof(double) + (2 * kOvMaxBlocks + 4) * sizeof(int32_t) +
                                (size_t)kOvMaxBlocks * kOvSlots * 3 * sizeof(float);
static_assert(kOvPartBytes % sizeof(double) == 0 && sizeof(OvHeader) == 32, "rows of doubles; the pinned header");
constexpr size_t ov_device_surv_bytes(int M, int B) { return (size_t)M * 2 * sizeof(float) * (size_t)(B + 1); }
constexpr size_t ov_pinned_bytes(int M, int B) { return (size_t)B * sizeof(OvHeader) + ov_device_surv_bytes(M, B); }
inline int ov_workgroups(int M) { return std::min((M + kBlock - 1) / kBlock, kOvMaxBlocks); }

struct OvRegions
{
  char *part;  // ov_part
  float *surv; // ov_surv
  char *host;  // ov_host
  int B;
};

__host__ __device__ inline void ov_bind_row(OvParams &P, const OvRegions &g, int row)
{
  char *part = g.part + (size_t)row * kOvPartBytes;
  P.part_motion = reinterpret_cast<double *>(part);
  P.part_count = reinterpret_cast<int32_t *>(part + kOvMaxBlocks * sizeof(double));
  int32_t *counters = P.part_count + 2 * kOvMaxBlocks;
  P.part_ext = reinterpret_cast<float *>(counters + 4);
  P.n_surv[0] = reinterpret_cast<int32_t *>(g.part + kOvMaxBlocks * sizeof(double)) + 2 * kOvMaxBlocks; // row 0's
  P.n_surv[1] = counters + 1;
  const size_t set = (size_t)P.M * 2;
  P.surv[0] = g.surv;
  P.surv[1] = g.surv + (size_t)(1 + row) * set;
  OvHeader *head = reinterpret_cast<OvHeader *>(g.host);
  P.host_head = head + row;
  P.host_surv[0] = reinterpret_cast<float *>(head + g.B);
  P.host_surv[1] = P.host_surv[0] + (size_t)(1 + row) * set;
}

// what the host fills for every row alike; the poses by value (the caller's are host memory)
struct OvBatchArgs
{
  OvParams P; // points, camera, mask, eps, M; the pose and the row's pointers are filled in per row (ov_row)
  OvRegions g;
  int nb;
  SageOverlapPose pose[SAGE_OVERLAP_MAX_BATCH];
};
static_assert(sizeof(OvBatchArgs) <= 4096, "kernel arguments");

__device__ __forceinline__ OvParams ov_row(const OvBatchArgs &A, int row)
{
  OvParams P = A.P;
  const SageOverlapPose &q = A.pose[row];
#pragma unroll
  for (int i = 0; i < 9; ++i)
    P.R[i] = q.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    P.t[i] = q.t[i];
  P.depth_scale = q.depth_scale;
  ov_bind_row(P, A.g, row);
  return P;
}

// grid (nb, B): row blockIdx.y is the single call with pose[blockIdx.y]; row 0 carries the input set too
__global__ __launch_bounds__(kBlock) void overlap_reduce_batch_kernel(const OvBatchArgs A)
{
  const OvParams P = ov_row(A, blockIdx.y);
  if (blockIdx.y == 0)
    ov_reduce_body<true>(P, blockIdx.x, gridDim.x);
  else
    ov_reduce_body<false>(P, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(kBlock) void overlap_filter_batch_kernel(const OvBatchArgs A)
{
  const OvParams P = ov_row(A, blockIdx.y);
  if (blockIdx.y == 0)
    ov_filter_body<true>(P, blockIdx.x, gridDim.x, A.nb);
  else
    ov_filter_body<false>(P, blockIdx.x, gridDim.x, A.nb);
}

// grid (B + 1): workgroup 0 publishes the input set and its count into every header, workgroup 1 + b the totals and the
// warped set of row b
__global__ __launch_bounds__(kBlock) void overlap_finish_batch_kernel(const OvBatchArgs A)
{
  const int tid = threadIdx.x;
  if (blockIdx.x == 0)
  {
    const OvParams P = ov_row(A, 0);
    const int c0 = ov_publish(P, 0, tid);
    if (tid < A.g.B)
      P.host_head[tid].n_cand[0] = c0;
    return;
  }
  const OvParams P = ov_row(A, blockIdx.x - 1);
  const int c1 = ov_publish(P, 1, tid);
  if (tid == 0)
  {
    ov_totals(P, A.nb);
    P.host_head->n_cand[1] = c1;
  }
}

bool ov_camera_ok(const SageCamera *cam)
{
  return std::isfinite(cam->fx) && std::isfinite(cam->fy) && cam->fx > 0.f && cam->fy > 0.f && std::isfinite(cam->w) &&
         std::isfinite(cam->h) && cam->w >= 1.f && cam->h >= 1.f && !(cam->w > 32768.f) && !(cam->h > 32768.f);
}

void ov_shared_params(OvParams &P, const float *dpts0_dev, const float *homo_dev, int M, const SageCamera *cam,
                      const float *mask_dev, float eps)
{
  P.dpts0 = dpts0_dev; P.homo = homo_dev; P.mask = mask_dev;
  P.eps = eps;
  P.fx = cam->fx; P.fy = cam->fy; P.cx = cam->cx; P.cy = cam->cy; P.w = cam->w; P.h = cam->h;
  P.W = (int)cam->w; P.H = (int)cam->h; P.M = M;
}

// the host half of one row: the hull of its warped set and the reference's three ratios (the input set's hull is given)
int ov_host_finish(const OvHeader *head, const float *host_warped, double input_area, int M, const SageCamera *cam,
                   SageOverlapStats *out)
{
  std::memset(out, 0, sizeof(*out));
  out->n_points = M;
  out->n_pos_depth = head->n_pos;
  out->n_in_mask = head->n_in;
  out->n_candidates[0] = head->n_cand[0];
  out->n_candidates[1] = head->n_cand[1];
  out->input_area = input_area;
  int rc;
  if ((rc = sage_convex_hull_area(host_warped, head->n_cand[1], &out->warp_area, nullptr)))
    return rc;
  out->area_ratio = (float)(out->warp_area / out->input_area); // 0 / 0: NaN, like the reference's float division
  out->inlier_ratio = (float)head->n_in / (float)M;
  // torch's mean of an empty tensor is NaN: 0.0 / 0
  const double mean = head->motion_sum / (double)head->n_pos;
  out->average_motion = (float)(mean / std::sqrt((double)cam->w * cam->w + (double)cam->h * cam->h));
  return SAGE_OK;
}
} // namespace

extern "C" int sage_track_overlap(SageWorkspace *ws, const float *R, const float *t, const float *dpts0_dev, float depth_scale,
                                  const float *homo_dev, int M, const SageCamera *cam, const float *mask_dev, float eps,
                                  SageOverlapStats *out)
{
  if (!ws || !R || !t || !dpts0_dev || !homo_dev || !cam || !mask_dev || !out || M <= 0)
    return SAGE_E_INVALID;
  if (!ov_camera_ok(cam))
    return SAGE_E_INVALID;
  int rc;
  if ((rc = ws->ov_part.reserve(kOvPartBytes)) || (rc = ws->ov_surv.reserve(ov_device_surv_bytes(M, 1))))
    return rc;
  // (every earlier call has been waited for: nobody writes the pinned region while it is replaced by a larger one)
  if ((rc = ws->ov_host.reserve(ov_pinned_bytes(M, 1))))
    return rc;
  OvParams P;
  std::memcpy(P.R, R, sizeof(P.R));
  std::memcpy(P.t, t, sizeof(P.t));
  P.depth_scale = depth_scale;
  ov_shared_params(P, dpts0_dev, homo_dev, M, cam, mask_dev, eps);
  ov_bind_row(P, OvRegions{ws->ov_part.as<char>(), ws->ov_surv.as<float>(), ws->ov_host.as<char>(), 1}, 0);
  const int nb = ov_workgroups(M);
  hipStream_t s = ws->stream;
  hipLaunchKernelGGL(overlap_reduce_kernel, dim3(nb), dim3(kBlock), 0, s, P);
  hipLaunchKernelGGL(overlap_filter_kernel, dim3(nb), dim3(kBlock), 0, s, P, nb);
  hipLaunchKernelGGL(overlap_finish_kernel, dim3(1), dim3(kBlock), 0, s, P, nb);
  SAGE_HIP(hipGetLastError());
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  double input_area;
  if ((rc = sage_convex_hull_area(P.host_surv[0], P.host_head->n_cand[0], &input_area, nullptr)))
    return rc;
  return ov_host_finish(P.host_head, P.host_surv[1], input_area, M, cam, out);
}

extern "C" int sage_track_overlap_batch_plan(int M, int B, int64_t *device_bytes, int64_t *pinned_bytes, int32_t *launches,
                                             int32_t *workgroups_per_row)
{
  if (B < 0 || B > SAGE_OVERLAP_MAX_BATCH || (B > 0 && M <= 0))
    return SAGE_E_INVALID;
  const int m = std::max(M, 0);
  if (device_bytes)
    *device_bytes = B ? (int64_t)((size_t)B * kOvPartBytes + ov_device_surv_bytes(m, B)) : 0;
  if (pinned_bytes)
    *pinned_bytes = B ? (int64_t)ov_pinned_bytes(m, B) : 0;
  if (launches)
    *launches = B ? 3 : 0;
  if (workgroups_per_row)
    *workgroups_per_row = m ? ov_workgroups(m) : 0;
  return SAGE_OK;
}

extern "C" int sage_track_overlap_batch_launches(const SageWorkspace *ws) { return ws ? ws->ov_batch_launches : 0; }

extern "C" int sage_track_overlap_batch(SageWorkspace *ws, const SageOverlapPose *poses, int B, const float *dpts0_dev,
                                        const float *homo_dev, int M, const SageCamera *cam, const float *mask_dev, float eps,
                                        SageOverlapStats *out)
{
  if (!ws || B < 0 || B > SAGE_OVERLAP_MAX_BATCH)
    return SAGE_E_INVALID;
  ws->ov_batch_launches = 0;
  if (B == 0)
    return SAGE_OK;
  if (!poses || !dpts0_dev || !homo_dev || !cam || !mask_dev || !out || M <= 0 || !ov_camera_ok(cam))
    return SAGE_E_INVALID;
  int rc;
  if ((rc = ws->ov_part.reserve((size_t)B * kOvPartBytes)) || (rc = ws->ov_surv.reserve(ov_device_surv_bytes(M, B))))
    return rc;
  // (every earlier call has been waited for: nobody writes the pinned region while it is replaced by a larger one)
  if ((rc = ws->ov_host.reserve(ov_pinned_bytes(M, B))))
    return rc;
  OvBatchArgs A;
  std::memset(&A.P, 0, sizeof(A.P));
  ov_shared_params(A.P, dpts0_dev, homo_dev, M, cam, mask_dev, eps);
  A.g = OvRegions{ws->ov_part.as<char>(), ws->ov_surv.as<float>(), ws->ov_host.as<char>(), B};
  A.nb = ov_workgroups(M);
  std::memcpy(A.pose, poses, (size_t)B * sizeof(SageOverlapPose));
  std::memset(A.pose + B, 0, (size_t)(SAGE_OVERLAP_MAX_BATCH - B) * sizeof(SageOverlapPose));
  hipStream_t s = ws->stream;
  hipLaunchKernelGGL(overlap_reduce_batch_kernel, dim3(A.nb, B), dim3(kBlock), 0, s, A);
  hipLaunchKernelGGL(overlap_filter_batch_kernel, dim3(A.nb, B), dim3(kBlock), 0, s, A);
  hipLaunchKernelGGL(overlap_finish_batch_kernel, dim3(B + 1), dim3(kBlock), 0, s, A);
  SAGE_HIP(hipGetLastError());
  ws->ov_batch_launches = 3;
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  // the input set once, then every row's own
  OvParams P = A.P;
  ov_bind_row(P, A.g, 0);
  double input_area;
  if ((rc = sage_convex_hull_area(P.host_surv[0], P.host_head->n_cand[0], &input_area, nullptr)))
    return rc;
  for (int b = 0; b < B; ++b)
  {
    ov_bind_row(P, A.g, b);
    if ((rc = ov_host_finish(P.host_head, P.host_surv[1], input_area, M, cam, out + b)))
      return rc;
  }
  return SAGE_OK;
}

