// registration.hip -- robust registration of keypoint matches: sage_robust_registration and sage_match_points.
// teaser::RobustRegistrationSolver::solve(src, dst, noise_bounds) in the reference's shipped configuration spends almost all of
// its time in the scale vote over the N (N - 1) / 2 pairs (registration.cc:395-485, :297-313, :21-88): 130 816 pairs at
// N = 512, a std::sort of twice as many interval endpoints and one sequential pass of six running sums.  Here the vote is
//
//   reg_pair_kernel        one lane per pair (i < j), the reference's pair order: in fp64 X = |dst_j - dst_i| / |src_j - src_i|,
//                          r = ((nb_i + nb_j) sqrt(cbar2)) (1 / |src_j - src_i|); writes (X, r) and the two endpoints X - r
//                          (entering), X + r (leaving) as order-preserving 64-bit keys with the payload 2 pair + leaving.  A
//                          pair without a usable measurement (v1 == 0; X or r not finite; r <= 0) writes padding instead and
//                          is counted.  The slots up to P, the power of two the sort runs over, are padded as well
//   reg_sort_tile_kernel,  a bitonic sort of (key, payload) pairs by key, ties by payload: all stages with a distance below a
//   reg_sort_stage_kernel, tile of 1024 endpoints run in LDS (12 KiB), the others two per launch (a lane per four endpoints; an
//   reg_sort_stage2_kernel odd one out alone).  Chosen over a radix sort for what it does not need: no histograms, no second
//                          copy of the endpoints, no order among workgroups; the result is a function of the multiset of
//                          (key, payload) alone
//   reg_tile_sums_kernel,  the running sums of e w, e w X, e r, e X, e X^2, the entering r and e (e = +1 entering, -1 leaving)
//   reg_tile_offsets_kernel, in fp64 over the sorted endpoints in three phases: per-tile totals, one workgroup's exclusive scan
//   reg_cost_kernel        of them, and per tile the inclusive sums with, fused, the vote's cost at every endpoint and the
//                          tile's first smallest one.  Every sum runs in a fixed order (lane-sequential, then a wave scan,
//                          then the waves, then the tiles): the same inputs give the same bytes on any workspace
//   reg_count_kernel       the first smallest cost over the tiles gives the scale; one lane per pair counts |X - scale| <= r
//   reg_publish_kernel     one workgroup: scale, cost and the counts, and the N points with their bounds (what the host
//                          finish reads), into the workspace's pinned record; posts the ticket
// then registration_host.cpp's finish on the host (O(N), fp64) -- or, where the workspace asks for it
// (SAGE_REG_FINISH_DEVICE), reg_finish_kernel below: the same finish, one workgroup per problem.  No float atomics (two integer counters), no workgroup
// waits for another, every loop is bounded by N, the tile or the number of tiles.  All stores are plain C++.
// Every kernel is a thin wrapper around a __device__ body that takes ONE problem's arrays and an index into them; the batched
// kernels (sage_robust_registration_batch, sage_match_points_batch: "the batched vote" below) call the same bodies over
// (problem, block) items, the problems lying as segments in the same allocations (the layout: registration_host.cpp).
#include "runtime_internal.h"
#include "registration_math.h"

namespace
{
constexpr int kRegTile = 2048;                  // endpoints per workgroup of the scan
constexpr int kSortTileMax = 4096;              // endpoints per workgroup of the sort's LDS stages: 1024, 2048 or 4096
                                                // the default, registration_sort_tile(), is 1024
                                                // (12 bytes of LDS each.  Measured at N = 512: 0.307 / 0.329 / 0.440 ms per call with 1024 /
                                                // 2048 / 4096 -- the LDS stages are what takes the time, and small tiles spread them over
                                                // more CUs; SAGE_REG_SORT_TILE picks another: scripts/registration_bench.py)
constexpr int kRegPerLane = kRegTile / kBlock;  // 8 consecutive endpoints per lane of the scan
constexpr int kRegQ = 7;                        // scanned quantities: e w, e w X, e r, e X, e X^2, [entering] r, e
constexpr int kRegRow = 8;                      // doubles per tile row (kRegQ + 1 unused: 64-byte rows)
constexpr uint32_t kRegPadPayload = 0xffffffffu;
constexpr uint64_t kRegPadKey = ~0ull;
constexpr int kRegNoIndex = 0x7fffffff;

struct RegHost // the pinned record
{
  double scale, scale_cost;
  int32_t n_pairs, n_degenerate, n_scale_inliers, vote_valid;
  int32_t M;         // sage_match_points: keypoints kept ...
  float mean_depth;  // ... and the mean of the depths the bounds were made from
  int32_t pad[6];
  float pts[1]; // src [N][3], dst [N][3], noise bounds [N]; then the translation inliers [N] int32 (written by the host)
};
static_assert(offsetof(RegHost, pts) == 64, "device-visible layout");

struct RegMin // a tile's (or the vote's) first smallest cost
{
  double cost, x;
  int idx; // position among the sorted endpoints; kRegNoIndex: none
};

struct RegTileMin // RegMin as stored per tile: 32 bytes
{
  double cost, x;
  long long idx;
  long long pad;
};

__device__ __forceinline__ uint64_t reg_key(double v)
{
  if (v == 0.0)
    v = 0.0; // (-0 and +0 are one value)
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ int reg_row_start(int i, int N) { return i * N - i * (i + 1) / 2; }

// pair p of one problem (keys, payload, pairs, counters: that problem's): its measurement, its two endpoints
__device__ __forceinline__ void reg_pair_body(const float *__restrict__ src, const float *__restrict__ dst,
                                              const float *__restrict__ nb, int N, int n_pairs, int half_P, double sqrt_cbar2,
                                              uint64_t *keys, uint32_t *payload, double2 *pairs, int *counters, int p)
{
#pragma clang fp contract(off) // the reference's operations one by one: no fused multiply-add
  if (p >= half_P)
    return;
  uint64_t k0 = kRegPadKey, k1 = kRegPadKey;
  uint32_t q0 = kRegPadPayload, q1 = kRegPadPayload;
  if (p < n_pairs)
  {
    // the row i with row_start(i) <= p < row_start(i + 1): the closed form, then the neighbours (the square root may be off)
    const double b = 2.0 * N - 1.0;
    int i = (int)((b - sqrt(fmax(b * b - 8.0 * (double)p, 0.0))) * 0.5);
    i = min(max(i, 0), N - 2);
    while (i > 0 && reg_row_start(i, N) > p)
      --i;
    while (i < N - 2 && reg_row_start(i + 1, N) <= p)
      ++i;
    const int j = p - reg_row_start(i, N) + i + 1;
    const double sx = (double)src[3 * j + 0] - (double)src[3 * i + 0], sy = (double)src[3 * j + 1] - (double)src[3 * i + 1],
                 sz = (double)src[3 * j + 2] - (double)src[3 * i + 2];
    const double dx = (double)dst[3 * j + 0] - (double)dst[3 * i + 0], dy = (double)dst[3 * j + 1] - (double)dst[3 * i + 1],
                 dz = (double)dst[3 * j + 2] - (double)dst[3 * i + 2];
    const double v1 = sqrt(sx * sx + sy * sy + sz * sz), v2 = sqrt(dx * dx + dy * dy + dz * dz);
    const double X = v2 / v1;
    const double r = (((double)nb[j] + (double)nb[i]) * sqrt_cbar2) * (1.0 / v1);
    const bool ok = v1 > 0.0 && isfinite(X) && isfinite(r) && r > 0.0 && isfinite(1.0 / (r * r));
    if (ok)
    {
      k0 = reg_key(X - r);
      k1 = reg_key(X + r);
      q0 = 2u * (uint32_t)p;
      q1 = q0 + 1u;
      pairs[p] = make_double2(X, r);
    }
    else
    {
      const double nan = __longlong_as_double(0x7ff8000000000000ll);
      pairs[p] = make_double2(nan, nan);
      atomicAdd(&counters[0], 1); // (rare)
    }
  }
  reinterpret_cast<ulonglong2 *>(keys)[p] = make_ulonglong2(k0, k1);
  reinterpret_cast<uint2 *>(payload)[p] = make_uint2(q0, q1);
}

__global__ __launch_bounds__(kBlock) void reg_pair_kernel(const float *__restrict__ src, const float *__restrict__ dst,
                                                          const float *__restrict__ nb, int N, int n_pairs, int half_P,
                                                          double sqrt_cbar2, uint64_t *keys, uint32_t *payload, double2 *pairs,
                                                          int *counters)
{
  reg_pair_body(src, dst, nb, N, n_pairs, half_P, sqrt_cbar2, keys, payload, pairs, counters, blockIdx.x * kBlock + threadIdx.x);
}

__device__ __forceinline__ bool reg_after(uint64_t ka, uint32_t pa, uint64_t kb, uint32_t pb)
{
  return ka > kb || (ka == kb && pa > pb);
}

// the bitonic network's stages k_first .. k_last (powers of two), each from the distance min(k / 2, kSortTile / 2) down to 1, on
// one tile in LDS (keys, payload: the tile's).  The direction of a compare-exchange comes from the endpoint's position in
// its own problem: base is the tile's first
template <int kSortTile>
__device__ __forceinline__ void reg_sort_tile_body(uint64_t *keys, uint32_t *payload, int base, int k_first, int k_last, uint64_t *s_k,
                                                   uint32_t *s_p)
{
  const int tid = threadIdx.x;
  for (int q = tid; q < kSortTile; q += kBlock)
  {
    s_k[q] = keys[q];
    s_p[q] = payload[q];
  }
  __syncthreads();
  for (int k = k_first; k <= k_last; k <<= 1)
    for (int j = min(k >> 1, kSortTile >> 1); j > 0; j >>= 1)
    {
      for (int t = tid; t < kSortTile / 2; t += kBlock)
      {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const bool up = ((base + lo) & k) == 0;
        const uint64_t ka = s_k[lo], kb = s_k[hi];
        const uint32_t pa = s_p[lo], pb = s_p[hi];
        if (reg_after(ka, pa, kb, pb) == up)
        {
          s_k[lo] = kb;
          s_k[hi] = ka;
          s_p[lo] = pb;
          s_p[hi] = pa;
        }
      }
      __syncthreads();
    }
  for (int q = tid; q < kSortTile; q += kBlock)
  {
    keys[q] = s_k[q];
    payload[q] = s_p[q];
  }
}

template <int kSortTile>
__global__ __launch_bounds__(kBlock) void reg_sort_tile_kernel(uint64_t *keys, uint32_t *payload, int k_first, int k_last)
{
  __shared__ uint64_t s_k[kSortTile];
  __shared__ uint32_t s_p[kSortTile];
  const int base = blockIdx.x * kSortTile;
  reg_sort_tile_body<kSortTile>(keys + base, payload + base, base, k_first, k_last, s_k, s_p);
}

// one stage (k, j) across tiles: compare-exchange t.  top: k is the problem's own P, its last stage, which sorts upwards
// wherever the problem lies (below its P the bit k of a position is the same in the problem and in the allocation: a
// problem starts at a multiple of its P)
__device__ __forceinline__ void reg_sort_stage_body(uint64_t *keys, uint32_t *payload, int k, int j, int t, bool top)
{
  const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
  const bool up = top || (lo & k) == 0;
  const uint64_t ka = keys[lo], kb = keys[hi];
  const uint32_t pa = payload[lo], pb = payload[hi];
  if (reg_after(ka, pa, kb, pb) == up)
  {
    keys[lo] = kb;
    keys[hi] = ka;
    payload[lo] = pb;
    payload[hi] = pa;
  }
}

__global__ __launch_bounds__(kBlock) void reg_sort_stage_kernel(uint64_t *keys, uint32_t *payload, int k, int j, int half_P)
{
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= half_P)
    return;
  reg_sort_stage_body(keys, payload, k, j, t, false); // (lo < P: the bit P is clear)
}

// two stages (k, j) and (k, j / 2) across tiles: four endpoints i0, i0 + j / 2, i0 + j, i0 + j + j / 2
// (i0: t with two zero bits inserted at j / 2 and j; k > j, so the four share a direction).  top: as above
__device__ __forceinline__ void reg_sort_stage2_body(uint64_t *keys, uint32_t *payload, int k, int j, int t, bool top)
{
  const int h = j >> 1;
  const int i0 = ((t & ~(h - 1)) << 2) | (t & (h - 1));
  const bool up = top || (i0 & k) == 0;
  const int at[4] = {i0, i0 + h, i0 + j, i0 + j + h};
  uint64_t kk[4];
  uint32_t pp[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    kk[q] = keys[at[q]];
    pp[q] = payload[at[q]];
  }
  auto exchange = [&](int a, int b) {
    if (reg_after(kk[a], pp[a], kk[b], pp[b]) == up)
    {
      const uint64_t tk = kk[a];
      kk[a] = kk[b];
      kk[b] = tk;
      const uint32_t tp = pp[a];
      pp[a] = pp[b];
      pp[b] = tp;
    }
  };
  exchange(0, 2); // distance j
  exchange(1, 3);
  exchange(0, 1); // distance j / 2
  exchange(2, 3);
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    keys[at[q]] = kk[q];
    payload[at[q]] = pp[q];
  }
}

__global__ __launch_bounds__(kBlock) void reg_sort_stage2_kernel(uint64_t *keys, uint32_t *payload, int k, int j, int quarter_P)
{
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= quarter_P)
    return;
  reg_sort_stage2_body(keys, payload, k, j, t, false);
}

// what one sorted endpoint adds to the running sums
__device__ __forceinline__ void reg_term(uint32_t pl, const double2 *__restrict__ pairs, double (&q)[kRegQ])
{
#pragma clang fp contract(off)
  if (pl == kRegPadPayload)
  {
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
      q[c] = 0.0;
    return;
  }
  const double2 m = pairs[pl >> 1];
  const double X = m.x, r = m.y;
  const bool entering = (pl & 1u) == 0u;
  const double e = entering ? 1.0 : -1.0;
  const double ew = e * (1.0 / (r * r));
  q[0] = ew;
  q[1] = ew * X;
  q[2] = e * r;
  q[3] = e * X;
  q[4] = (e * X) * X;
  q[5] = entering ? r : 0.0;
  q[6] = e;
}

// v: this lane's totals.  -> excl: the totals of the lanes before it in the workgroup; total: the workgroup's.  Fixed order:
// an inclusive wave scan (log steps), then the waves in turn.  s_wave [kWaves][kRegQ]; ends behind a barrier
__device__ __forceinline__ void reg_block_scan(const double (&v)[kRegQ], double (&excl)[kRegQ], double (&total)[kRegQ],
                                               double (*s_wave)[kRegQ])
{
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double before[kRegQ];
#pragma unroll
  for (int c = 0; c < kRegQ; ++c)
  {
    double inc = v[c];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
      const double t = __shfl_up(inc, o, 64);
      if (lane >= o)
        inc += t;
    }
    const double prev = __shfl_up(inc, 1, 64);
    before[c] = lane ? prev : 0.0;
    if (lane == 63)
      s_wave[wave][c] = inc;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kRegQ; ++c)
  {
    double off = 0.0, tot = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
    {
      if (w < wave)
        off += s_wave[w][c];
      tot += s_wave[w][c];
    }
    excl[c] = off + before[c];
    total[c] = tot;
  }
  __syncthreads();
}

// tile `tile` of one problem (payload, pairs, tile_sums: that problem's): the totals of its 2048 endpoints
__device__ __forceinline__ void reg_tile_sums_body(const uint32_t *__restrict__ payload, const double2 *__restrict__ pairs,
                                                   double *tile_sums, int tile, double (*s_wave)[kRegQ])
{
#pragma clang fp contract(off)
  const int at = tile * kRegTile + threadIdx.x * kRegPerLane;
  double v[kRegQ] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < kRegPerLane; ++e)
  {
    double q[kRegQ];
    reg_term(payload[at + e], pairs, q);
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
      v[c] += q[c];
  }
  double excl[kRegQ], total[kRegQ];
  reg_block_scan(v, excl, total, s_wave);
  if (threadIdx.x == 0)
  {
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
      tile_sums[(size_t)tile * kRegRow + c] = total[c];
  }
}

__global__ __launch_bounds__(kBlock) void reg_tile_sums_kernel(const uint32_t *__restrict__ payload, const double2 *__restrict__ pairs,
                                                               double *tile_sums)
{
  __shared__ double s_wave[kWaves][kRegQ];
  reg_tile_sums_body(payload, pairs, tile_sums, blockIdx.x, s_wave);
}

// one workgroup per problem: tile_offs[t] = the sums of the tiles before t, tile_offs[n_tiles] = the sums of all
__device__ __forceinline__ void reg_tile_offsets_body(const double *__restrict__ tile_sums, double *tile_offs, int n_tiles,
                                                      double (*s_wave)[kRegQ])
{
#pragma clang fp contract(off)
  const int per = (n_tiles + kBlock - 1) / kBlock;
  const int t0 = min(threadIdx.x * per, n_tiles), t1 = min(t0 + per, n_tiles);
  double v[kRegQ] = {0, 0, 0, 0, 0, 0, 0};
  for (int t = t0; t < t1; ++t)
  {
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
      v[c] += tile_sums[(size_t)t * kRegRow + c];
  }
  double run[kRegQ], total[kRegQ];
  reg_block_scan(v, run, total, s_wave);
  for (int t = t0; t < t1; ++t)
  {
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
    {
      tile_offs[(size_t)t * kRegRow + c] = run[c];
      run[c] += tile_sums[(size_t)t * kRegRow + c];
    }
  }
  if (threadIdx.x == 0)
  {
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
      tile_offs[(size_t)n_tiles * kRegRow + c] = total[c];
  }
}

__global__ __launch_bounds__(kBlock) void reg_tile_offsets_kernel(const double *__restrict__ tile_sums, double *tile_offs, int n_tiles)
{
  __shared__ double s_wave[kWaves][kRegQ];
  reg_tile_offsets_body(tile_sums, tile_offs, n_tiles, s_wave);
}

__device__ __forceinline__ bool reg_min_before(const RegMin &a, const RegMin &b) // a wins over b: smaller cost, then earlier
{
  return a.cost < b.cost || (a.cost == b.cost && a.idx < b.idx);
}

// the workgroup's first smallest; valid in every thread.  s_min [kWaves]; ends behind a barrier
__device__ __forceinline__ RegMin reg_block_min(RegMin m, RegMin *s_min)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    RegMin other;
    other.cost = __shfl_down(m.cost, o, 64);
    other.x = __shfl_down(m.x, o, 64);
    other.idx = __shfl_down(m.idx, o, 64);
    if (reg_min_before(other, m))
      m = other;
  }
  if ((threadIdx.x & 63) == 0)
    s_min[threadIdx.x >> 6] = m;
  __syncthreads();
  RegMin best = s_min[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
    if (reg_min_before(s_min[w], best))
      best = s_min[w];
  __syncthreads();
  return best;
}

// per tile: the inclusive running sums at every endpoint, the vote's cost there, the tile's first smallest cost.  A NaN cost
// (an empty consensus set: 0 / 0) never wins
__device__ __forceinline__ void reg_cost_body(const uint32_t *__restrict__ payload, const double2 *__restrict__ pairs,
                                              const double *__restrict__ tile_offs, int n_tiles, RegTileMin *tile_min, int tile,
                                              double (*s_wave)[kRegQ], RegMin *s_min)
{
#pragma clang fp contract(off)
  const int at = tile * kRegTile + threadIdx.x * kRegPerLane;
  uint32_t pl[kRegPerLane];
  double v[kRegQ] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < kRegPerLane; ++e)
  {
    pl[e] = payload[at + e];
    double q[kRegQ];
    reg_term(pl[e], pairs, q);
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
      v[c] += q[c];
  }
  double run[kRegQ], total[kRegQ];
  reg_block_scan(v, run, total, s_wave);
#pragma unroll
  for (int c = 0; c < kRegQ; ++c)
    run[c] = tile_offs[(size_t)tile * kRegRow + c] + run[c];
  const double r_all = tile_offs[(size_t)n_tiles * kRegRow + 5];
  RegMin best;
  best.cost = __longlong_as_double(0x7ff0000000000000ll); // +inf
  best.x = 0.0;
  best.idx = kRegNoIndex;
#pragma unroll
  for (int e = 0; e < kRegPerLane; ++e)
  {
    double q[kRegQ];
    reg_term(pl[e], pairs, q);
#pragma unroll
    for (int c = 0; c < kRegQ; ++c)
      run[c] += q[c];
    if (pl[e] != kRegPadPayload)
    {
      const double x = run[1] / run[0];
      const double residual = (run[6] * x) * x + run[4] - (2.0 * run[3]) * x;
      const double cost = residual + (r_all - run[2]);
      if (cost < best.cost) // (false for a NaN; the first of equal costs stays)
      {
        best.cost = cost;
        best.x = x;
        best.idx = at + e;
      }
    }
  }
  best = reg_block_min(best, s_min);
  if (threadIdx.x == 0)
  {
    RegTileMin out;
    out.cost = best.cost;
    out.x = best.x;
    out.idx = best.idx;
    out.pad = 0;
    tile_min[tile] = out;
  }
}

__global__ __launch_bounds__(kBlock) void reg_cost_kernel(const uint32_t *__restrict__ payload, const double2 *__restrict__ pairs,
                                                          const double *__restrict__ tile_offs, int n_tiles, RegTileMin *tile_min)
{
  __shared__ double s_wave[kWaves][kRegQ];
  __shared__ RegMin s_min[kWaves];
  reg_cost_body(payload, pairs, tile_offs, n_tiles, tile_min, blockIdx.x, s_wave, s_min);
}

// the first smallest cost over the tiles; valid in every thread
__device__ __forceinline__ RegMin reg_vote_min(const RegTileMin *__restrict__ tile_min, int n_tiles, RegMin *s_min)
{
  RegMin m;
  m.cost = __longlong_as_double(0x7ff0000000000000ll);
  m.x = 0.0;
  m.idx = kRegNoIndex;
  for (int t = threadIdx.x; t < n_tiles; t += kBlock)
  {
    RegMin o;
    o.cost = tile_min[t].cost;
    o.x = tile_min[t].x;
    o.idx = (int)tile_min[t].idx;
    if (reg_min_before(o, m))
      m = o;
  }
  return reg_block_min(m, s_min);
}

// pair p of one problem against that problem's vote
__device__ __forceinline__ void reg_count_body(const double2 *__restrict__ pairs, int n_pairs, const RegTileMin *__restrict__ tile_min,
                                               int n_tiles, int *counters, int p, RegMin *s_min)
{
  const RegMin vote = reg_vote_min(tile_min, n_tiles, s_min);
  if (vote.idx == kRegNoIndex)
    return; // (uniform)
  bool in = false;
  if (p < n_pairs)
  {
    const double2 m = pairs[p];
    in = fabs(m.x - vote.x) <= m.y; // (false for a pair that left the vote: NaN)
  }
  const int n = __popcll(__ballot(in));
  if ((threadIdx.x & 63) == 0 && n)
    atomicAdd(&counters[1], n);
}

__global__ __launch_bounds__(kBlock) void reg_count_kernel(const double2 *__restrict__ pairs, int n_pairs,
                                                           const RegTileMin *__restrict__ tile_min, int n_tiles, int *counters)
{
  __shared__ RegMin s_min[kWaves];
  reg_count_body(pairs, n_pairs, tile_min, n_tiles, counters, blockIdx.x * kBlock + threadIdx.x, s_min);
}

// one workgroup per problem: its pinned record; ends behind a system fence and a barrier
__device__ __forceinline__ void reg_publish_body(const float *__restrict__ src, const float *__restrict__ dst,
                                                 const float *__restrict__ nb, int N, int n_pairs,
                                                 const RegTileMin *__restrict__ tile_min, int n_tiles,
                                                 const int *__restrict__ counters, RegHost *host, RegMin *s_min)
{
  const RegMin vote = reg_vote_min(tile_min, n_tiles, s_min);
  const int tid = threadIdx.x;
  for (int q = tid; q < 3 * N; q += kBlock)
  {
    host->pts[q] = src[q];
    host->pts[3 * N + q] = dst[q];
  }
  for (int q = tid; q < N; q += kBlock)
    host->pts[6 * N + q] = nb[q];
  if (tid == 0)
  {
    host->scale = vote.x;
    host->scale_cost = vote.cost;
    host->n_pairs = n_pairs;
    host->n_degenerate = counters[0];
    host->n_scale_inliers = counters[1];
    host->vote_valid = vote.idx != kRegNoIndex;
  }
  __threadfence_system();
  __syncthreads();
}

__global__ __launch_bounds__(kBlock) void reg_publish_kernel(const float *__restrict__ src, const float *__restrict__ dst,
                                                             const float *__restrict__ nb, int N, int n_pairs,
                                                             const RegTileMin *__restrict__ tile_min, int n_tiles,
                                                             const int *__restrict__ counters, RegHost *host,
                                                             volatile unsigned *ticket, unsigned epoch)
{
  __shared__ RegMin s_min[kWaves];
  reg_publish_body(src, dst, nb, N, n_pairs, tile_min, n_tiles, counters, host, s_min);
  if (threadIdx.x == 0)
  {
    __threadfence_system();
    *ticket = epoch;
  }
}

// ---- the batched vote (sage_robust_registration_batch): the kernels above over (problem, block) items ----
// The voting problems are segments of the keys / payload / pairs allocations, by descending P (registration_plan.h), so a
// segment starts at a multiple of its own P and of every tile size: block b of a sort launch IS the allocation's tile b, and
// the compare-exchange t of a cross-tile stage IS the allocation's; only the direction of the last stage (k = the
// segment's own P) needs the segment.  A stage with k concerns the segments with P >= k, a prefix of the allocation, and
// is launched over that prefix.  A workgroup finds its segment in the table below (a kernel argument; at most 32 rows,
// the lookup is uniform)
struct RegSegTable
{
  int n;
  int start[SAGE_REG_MAX_BATCH + 1];   // first endpoint; [n]: the total
  int tile0[SAGE_REG_MAX_BATCH + 1];   // scan tiles before the segment
  int cblock0[SAGE_REG_MAX_BATCH + 1]; // 256-pair blocks before the segment
  int pair0[SAGE_REG_MAX_BATCH], N[SAGE_REG_MAX_BATCH], n_pairs[SAGE_REG_MAX_BATCH], n_tiles[SAGE_REG_MAX_BATCH];
  long long rows0[SAGE_REG_MAX_BATCH]; // the segment's tile rows, bytes into the tiles allocation
};
struct RegSegPoints // the problems' inputs and pinned records, in segment order
{
  const float *src[SAGE_REG_MAX_BATCH], *dst[SAGE_REG_MAX_BATCH], *nb[SAGE_REG_MAX_BATCH];
  RegHost *host[SAGE_REG_MAX_BATCH];
};

// the s with first[s] <= v < first[s + 1]
__device__ __forceinline__ int reg_segment_of(const int (&first)[SAGE_REG_MAX_BATCH + 1], int n, int v)
{
  int s = 0;
  while (s + 1 < n && first[s + 1] <= v)
    ++s;
  return s;
}

struct RegSegRows // a segment's part of the tiles allocation
{
  double *sums, *offs;
  RegTileMin *min;
  int *counters;
};
__device__ __forceinline__ RegSegRows reg_segment_rows(const RegSegTable &T, int s, char *tiles)
{
  const size_t nt = (size_t)T.n_tiles[s];
  RegSegRows r;
  char *rows = tiles + T.rows0[s];
  r.sums = reinterpret_cast<double *>(rows);
  r.offs = reinterpret_cast<double *>(rows + nt * kRegRow * sizeof(double));
  r.min = reinterpret_cast<RegTileMin *>(rows + (2 * nt + 1) * kRegRow * sizeof(double));
  r.counters = reinterpret_cast<int *>(tiles) + 4 * s;
  return r;
}

// grid: total endpoints / 512
__global__ __launch_bounds__(kBlock) void reg_pair_batch_kernel(const RegSegTable T, const RegSegPoints Q, double sqrt_cbar2, uint64_t *keys,
                                                                uint32_t *payload, double2 *pairs, char *tiles)
{
  const int s = reg_segment_of(T.start, T.n, blockIdx.x * (2 * kBlock));
  const int start = T.start[s], half_P = (T.start[s + 1] - start) >> 1;
  reg_pair_body(Q.src[s], Q.dst[s], Q.nb[s], T.N[s], T.n_pairs[s], half_P, sqrt_cbar2, keys + start, payload + start, pairs + T.pair0[s],
                reinterpret_cast<int *>(tiles) + 4 * s, blockIdx.x * kBlock + threadIdx.x - (start >> 1));
}

// grid: (the endpoints of the segments with P >= k_last) / kSortTile
template <int kSortTile>
__global__ __launch_bounds__(kBlock) void reg_sort_tile_batch_kernel(const RegSegTable T, uint64_t *keys, uint32_t *payload, int k_first,
                                                                     int k_last)
{
  __shared__ uint64_t s_k[kSortTile];
  __shared__ uint32_t s_p[kSortTile];
  const int base = blockIdx.x * kSortTile;
  const int s = reg_segment_of(T.start, T.n, base);
  reg_sort_tile_body<kSortTile>(keys + base, payload + base, base - T.start[s], k_first, k_last, s_k, s_p);
}

// grid: (the endpoints of the segments with P >= k) / 512
__global__ __launch_bounds__(kBlock) void reg_sort_stage_batch_kernel(const RegSegTable T, uint64_t *keys, uint32_t *payload, int k, int j)
{
  const int s = reg_segment_of(T.start, T.n, blockIdx.x * (2 * kBlock));
  reg_sort_stage_body(keys, payload, k, j, blockIdx.x * kBlock + threadIdx.x, T.start[s + 1] - T.start[s] == k);
}

// grid: (the endpoints of the segments with P >= k) / 1024
__global__ __launch_bounds__(kBlock) void reg_sort_stage2_batch_kernel(const RegSegTable T, uint64_t *keys, uint32_t *payload, int k, int j)
{
  const int s = reg_segment_of(T.start, T.n, blockIdx.x * (4 * kBlock));
  reg_sort_stage2_body(keys, payload, k, j, blockIdx.x * kBlock + threadIdx.x, T.start[s + 1] - T.start[s] == k);
}

// grid: the segments' scan tiles
__global__ __launch_bounds__(kBlock) void reg_tile_sums_batch_kernel(const RegSegTable T, const uint32_t *__restrict__ payload,
                                                                     const double2 *__restrict__ pairs, char *tiles)
{
  __shared__ double s_wave[kWaves][kRegQ];
  const int s = reg_segment_of(T.tile0, T.n, blockIdx.x);
  reg_tile_sums_body(payload + T.start[s], pairs + T.pair0[s], reg_segment_rows(T, s, tiles).sums, blockIdx.x - T.tile0[s], s_wave);
}

// grid: the segments
__global__ __launch_bounds__(kBlock) void reg_tile_offsets_batch_kernel(const RegSegTable T, char *tiles)
{
  __shared__ double s_wave[kWaves][kRegQ];
  const RegSegRows r = reg_segment_rows(T, blockIdx.x, tiles);
  reg_tile_offsets_body(r.sums, r.offs, T.n_tiles[blockIdx.x], s_wave);
}

// grid: the segments' scan tiles
__global__ __launch_bounds__(kBlock) void reg_cost_batch_kernel(const RegSegTable T, const uint32_t *__restrict__ payload,
                                                                const double2 *__restrict__ pairs, char *tiles)
{
  __shared__ double s_wave[kWaves][kRegQ];
  __shared__ RegMin s_min[kWaves];
  const int s = reg_segment_of(T.tile0, T.n, blockIdx.x);
  const RegSegRows r = reg_segment_rows(T, s, tiles);
  reg_cost_body(payload + T.start[s], pairs + T.pair0[s], r.offs, T.n_tiles[s], r.min, blockIdx.x - T.tile0[s], s_wave, s_min);
}

// grid: the segments' 256-pair blocks
__global__ __launch_bounds__(kBlock) void reg_count_batch_kernel(const RegSegTable T, const double2 *__restrict__ pairs, char *tiles)
{
  __shared__ RegMin s_min[kWaves];
  const int s = reg_segment_of(T.cblock0, T.n, blockIdx.x);
  const RegSegRows r = reg_segment_rows(T, s, tiles);
  reg_count_body(pairs + T.pair0[s], T.n_pairs[s], r.min, T.n_tiles[s], r.counters, (blockIdx.x - T.cblock0[s]) * kBlock + threadIdx.x, s_min);
}

// grid: the segments.  The ticket comes behind this launch in the stream (ws_ticket_wait)
__global__ __launch_bounds__(kBlock) void reg_publish_batch_kernel(const RegSegTable T, const RegSegPoints Q, char *tiles)
{
  __shared__ RegMin s_min[kWaves];
  const int s = blockIdx.x;
  const RegSegRows r = reg_segment_rows(T, s, tiles);
  reg_publish_body(Q.src[s], Q.dst[s], Q.nb[s], T.N[s], T.n_pairs[s], r.min, T.n_tiles[s], r.counters, Q.host[s], s_min);
}

// rows of int32 out of pinned memory, one row per blockIdx.y: out[i] = map ? map[in[i]] : in[i].  The batch's inliers_dev rows
// (map NULL) and the pre-check's inlier keypoints (map: kept)
struct RegRowCopy
{
  const int32_t *in[SAGE_REG_MAX_BATCH];  // pinned
  const int32_t *map[SAGE_REG_MAX_BATCH]; // device, or NULL
  int32_t *out[SAGE_REG_MAX_BATCH];
  int n[SAGE_REG_MAX_BATCH];
};
__global__ __launch_bounds__(kBlock) void reg_row_copy_kernel(const RegRowCopy R)
{
  const int b = blockIdx.y, i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= R.n[b])
    return;
  const int32_t v = R.in[b][i];
  R.out[b][i] = R.map[b] ? R.map[b][v] : v;
}

struct MatchPointsParams
{
  const int32_t *flags;
  const int64_t *loc1;
  const float *dpts0, *homo0, *dpt_map_1;
  float divisor0, cx, cy, fx, fy, Wf, focal, mult;
  long long HW;
  int K, noise_from;
  float *pts0, *pts1, *noise_bounds, *homo1, *dpts1;
  int32_t *kept;
};

// a matched pixel of frame 1 -> its homogeneous coordinates and its depth (camera_tracker.cpp:654-678), in fp32 and in the
// reference's order of operations; a location outside the map reads a NaN depth.  Shared by the gather in front of the
// solver (reg_match_points_kernel) and the one in front of the tracker (verify_gather_kernel)
__device__ __forceinline__ void matched_point(long long loc, float Wf, float cx, float cy, float fx, float fy, long long HW,
                                              const float *__restrict__ dpt_map_1, float *hx, float *hy, float *d1)
{
#pragma clang fp contract(off)
  const float lf = (float)loc;
  const float x = fmodf(lf, Wf), y = floorf(lf / Wf);
  *hx = (x - cx) / fx;
  *hy = (y - cy) / fy;
  *d1 = (loc >= 0 && loc < HW) ? dpt_map_1[loc] : __int_as_float(0x7fc00000);
}

// one workgroup per problem: compacts the flagged keypoints in ascending order (a wave scan of the flags per 256 keypoints) and
// evaluates the gather's fp32 expressions for each; the depths' sum in fp64 (per lane, then the workgroup's tree).  Thread 0
// leaves the count and the mean in the pinned record, behind a system fence
__device__ __forceinline__ void reg_match_points_body(const MatchPointsParams &P, RegHost *host, int *s_cnt, double *s_sum)
{
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int total = 0; // the same in every thread
  double dsum = 0.0;
  for (int base = 0; base < P.K; base += kBlock)
  {
    const int k = base + tid;
    const bool keep = k < P.K && P.flags[k] != 0;
    int inc = keep ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o)
        inc += t;
    }
    if (lane == 63)
      s_cnt[wave] = inc;
    __syncthreads();
    int before = total, tile = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
    {
      if (w < wave)
        before += s_cnt[w];
      tile += s_cnt[w];
    }
    if (keep)
    {
      const int m = before + inc - 1;
      const float d0 = P.dpts0[k];
      const float s0 = d0 / P.divisor0;
      const float h0x = P.homo0[3 * k + 0], h0y = P.homo0[3 * k + 1], h0z = P.homo0[3 * k + 2];
      P.pts0[3 * m + 0] = s0 * h0x;
      P.pts0[3 * m + 1] = s0 * h0y;
      P.pts0[3 * m + 2] = s0 * h0z;
      float hx, hy, d1;
      matched_point(P.loc1[k], P.Wf, P.cx, P.cy, P.fx, P.fy, P.HW, P.dpt_map_1, &hx, &hy, &d1);
      P.homo1[3 * m + 0] = hx;
      P.homo1[3 * m + 1] = hy;
      P.homo1[3 * m + 2] = 1.0f;
      P.dpts1[m] = d1;
      P.pts1[3 * m + 0] = d1 * hx;
      P.pts1[3 * m + 1] = d1 * hy;
      P.pts1[3 * m + 2] = d1 * 1.0f;
      const float d = P.noise_from ? d1 : d0;
      const float b = (P.mult * d) / P.focal;
      P.noise_bounds[m] = b != b ? b : fmaxf(b, 5.0e-4f); // (clamp_min keeps a NaN)
      P.kept[m] = k;
      dsum += (double)d;
    }
    total += tile;
    __syncthreads(); // (s_cnt is written again)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    dsum += __shfl_down(dsum, o, 64);
  if (lane == 0)
    s_sum[wave] = dsum;
  __syncthreads();
  if (tid == 0)
  {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
      s += s_sum[w];
    host->M = total;
    host->mean_depth = total ? (float)(s / (double)total) : 0.0f;
    __threadfence_system();
  }
}

__global__ __launch_bounds__(kBlock) void reg_match_points_kernel(const MatchPointsParams P, RegHost *host, volatile unsigned *ticket,
                                                                  unsigned epoch)
{
  __shared__ int s_cnt[kWaves];
  __shared__ double s_sum[kWaves];
  reg_match_points_body(P, host, s_cnt, s_sum);
  if (threadIdx.x == 0)
    *ticket = epoch;
}

struct MatchPointsBatch
{
  SageMatchPointsItem item[SAGE_REG_MAX_BATCH];
  MatchPointsParams shared; // the scalars (the pointers are taken from the item)
  RegHost *host;            // [B] records of 64 bytes: problem b's count and mean
};
static_assert(sizeof(MatchPointsBatch) <= 4096, "a kernel argument");

// grid: the problems.  The ticket comes behind this launch in the stream (ws_ticket_wait)
__global__ __launch_bounds__(kBlock) void reg_match_points_batch_kernel(const MatchPointsBatch G)
{
  __shared__ int s_cnt[kWaves];
  __shared__ double s_sum[kWaves];
  const SageMatchPointsItem &it = G.item[blockIdx.x];
  MatchPointsParams P = G.shared;
  P.flags = it.cyc_inlier_flags; P.loc1 = it.raw_matched_loc1d_1; P.dpts0 = it.dpts0; P.homo0 = it.homo0; P.dpt_map_1 = it.dpt_map_1;
  P.pts0 = it.pts0; P.pts1 = it.pts1; P.noise_bounds = it.noise_bounds; P.homo1 = it.homo1; P.dpts1 = it.dpts1; P.kept = it.kept;
  reg_match_points_body(P, reinterpret_cast<RegHost *>(reinterpret_cast<char *>(G.host) + 64 * (size_t)blockIdx.x), s_cnt, s_sum);
}
} // namespace

// ---- the finish on the device (SAGE_REG_FINISH_DEVICE, sage_registration_finish_batch): reg_finish_kernel ----
// sage_registration_finish (registration_host.cpp) for one problem per workgroup of kBlock lanes, in fp64, its expressions
// literally and in its order; what differs is the order of the sums.  Point / chain TIM i belongs to lane i % kBlock (up to
// four per lane, ascending).  The phases:
//   entry        the problem's scale: the first smallest cost over the vote's tile minima (what reg_publish_body reads; every
//                wave finds it by itself with shuffles, no barrier), or the caller's.  An empty vote: lane 0 writes valid = 0,
//                the workgroup returns as one before any barrier
//   TIMs         ts, td = (dst_leaf - dst_i) (1 / scale) into LDS ([3][N] each: a lane reads back only what it wrote), the
//                squared bounds and the weights in registers
//   GNC          per iteration two barriers: the nine sums of H = sum (x w) y, then the cost sum w r^2 of the previous weights
//                (at iteration 0 with the largest r^2).  A sum: a lane's terms ascending, a shuffle tree over the wave, the
//                four waves ascending out of LDS -- a function of N alone.  Every lane reads the same totals and runs
//                registration_math.h's 3x3 SVD itself: R, mu, the cost and so every exit (mu <= 0, cost_diff < threshold, the
//                cap) are the same in all lanes, no barrier sits in a divergent branch
//   translation  per axis: raw = dst - (scale R) src and its range into LDS (over the TIMs, which are done), the 2 N endpoints
//                as (reg_key, 2 i + leaving) padded to the power of two P2 >= 2 N, a bitonic sort in LDS (ties by position:
//                the host's stable sort), then the scale vote's scan (reg_term, reg_block_scan), cost and first smallest
//                (reg_block_min) with P2 / kBlock consecutive endpoints per lane
//   outputs      the AND of the three masks compacted ascending (a wave scan of the flags per 256 points, as
//                reg_match_points_body) into the record's list and, if given, the problem's inliers_dev row (through the
//                pre-check's map when there is one); the rotation mask; R, t and the counts by lane 0
// Bounded: 60 Jacobi sweeps, rotation_max_iterations <= SAGE_REG_FINISH_MAX_ITERATIONS, a sort that does not look at the
// data.  Every index is below N (a payload is a position this workgroup wrote, or the padding).  All stores are plain C++.
namespace
{
constexpr int kFinPerLane = SAGE_REG_MAX_POINTS / kBlock; // points / TIMs per lane: i = tid + kBlock k
constexpr int kFinEnds = 2 * SAGE_REG_MAX_POINTS;        // endpoints of a translation vote at the cap: one scan tile
static_assert(kFinEnds == kRegTile && kFinEnds / kBlock == kRegPerLane, "a translation vote fits the scan's tile");

struct RegFinishHost // the finish's pinned record: 128 bytes, then the translation inliers [N] int32, the rotation mask [N] uint8
{
  double R[9], t[3];
  int32_t valid, n_inliers, rotation_iterations, n_rotation_inliers;
  int32_t pad[4];
};
static_assert(sizeof(RegFinishHost) == kRegFinishRecordHeader, "device-visible layout");

struct RegFinishItem // one problem
{
  const float *src, *dst, *nb;
  const RegTileMin *tile_min; // its vote's tile minima [n_tiles]; NULL: the scale is the caller's
  RegFinishHost *out;
  int32_t *inliers_dev;   // or NULL
  const int32_t *map;     // or NULL: inliers_dev receives map[inlier]
  double noise_bound, scale;
  int N, n_tiles;
};
struct RegFinishBatch
{
  RegFinishItem item[SAGE_REG_MAX_BATCH];
  double sqrt_cbar2, cost_threshold, gnc_factor;
  int max_iterations, pad;
};
static_assert(sizeof(RegFinishBatch) <= 4096, "a kernel argument");

struct alignas(16) RegFinishLds
{
  double tim[6 * SAGE_REG_MAX_POINTS]; // ts [3][1024] | td [3][1024]; then keys [2048] u64 | (X, r) [1024] | payload [2048] u32
  double H[kWaves][9];
  double cost[kWaves][2];
  double wave[kWaves][kRegQ];
  RegMin min[kWaves];
  int cnt[kWaves];
};
static_assert(sizeof(RegFinishLds) == kRegFinishLdsBytes, "what sage_registration_finish_plan reports");

// the vote's first smallest cost, found by every wave on its own (reg_min_before is a strict order: the answer is
// reg_vote_min's); no LDS, no barrier
__device__ __forceinline__ RegMin reg_vote_min_wave(const RegTileMin *__restrict__ tile_min, int n_tiles)
{
  RegMin m;
  m.cost = __longlong_as_double(0x7ff0000000000000ll);
  m.x = 0.0;
  m.idx = kRegNoIndex;
  for (int t = threadIdx.x & 63; t < n_tiles; t += 64)
  {
    RegMin o;
    o.cost = tile_min[t].cost;
    o.x = tile_min[t].x;
    o.idx = (int)tile_min[t].idx;
    if (reg_min_before(o, m))
      m = o;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    RegMin other;
    other.cost = __shfl_xor(m.cost, o, 64);
    other.x = __shfl_xor(m.x, o, 64);
    other.idx = __shfl_xor(m.idx, o, 64);
    if (reg_min_before(other, m))
      m = other;
  }
  return m;
}

// the workgroup's number of set flags; valid in every thread.  ends behind a barrier
__device__ __forceinline__ int reg_block_count(bool flag, int *s_cnt)
{
  const int n = __popcll(__ballot(flag));
  if ((threadIdx.x & 63) == 0)
    s_cnt[threadIdx.x >> 6] = n;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w)
    total += s_cnt[w];
  __syncthreads();
  return total;
}

__device__ __forceinline__ void reg_finish_body(const RegFinishItem &it, const RegFinishBatch &G, RegFinishLds &L)
{
#pragma clang fp contract(off) // the host's operations one by one
  using sage_reg::Mat3;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = it.N;
  const float *__restrict__ src = it.src, *__restrict__ dst = it.dst, *__restrict__ nbf = it.nb;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);

  // ---- entry
  double scale = it.scale;
  if (it.tile_min)
  {
    const RegMin vote = reg_vote_min_wave(it.tile_min, it.n_tiles);
    if (vote.idx == kRegNoIndex) // (the same in every lane: no pair was left in the vote)
    {
      if (tid == 0)
      {
        it.out->valid = 0;
        it.out->n_inliers = 0;
        it.out->rotation_iterations = 0;
        it.out->n_rotation_inliers = 0;
      }
      return;
    }
    scale = vote.x;
  }

  // ---- the chain TIMs
  double *s_ts = L.tim, *s_td = L.tim + 3 * SAGE_REG_MAX_POINTS;
  const double inv_scale = 1 / scale;
  double bsq[kFinPerLane], w[kFinPerLane];
#pragma unroll
  for (int k = 0; k < kFinPerLane; ++k)
  {
    const int i = tid + k * kBlock;
    bsq[k] = 0.0;
    w[k] = 1.0;
    if (i < n)
    {
      const int leaf = i != n - 1 ? i + 1 : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
      {
        s_ts[c * SAGE_REG_MAX_POINTS + i] = (double)src[3 * leaf + c] - (double)src[3 * i + c];
        s_td[c * SAGE_REG_MAX_POINTS + i] = ((double)dst[3 * leaf + c] - (double)dst[3 * i + c]) * inv_scale;
      }
      const double tb = ((double)nbf[leaf] + (double)nbf[i]) * inv_scale;
      bsq[k] = tb * tb;
    }
  }
  const double gnc_bound = it.noise_bound * (2 / scale);
  double noise_bound_sq = gnc_bound * gnc_bound;
  if (noise_bound_sq < 1e-16)
    noise_bound_sq = 1e-2;

  // ---- GNC-TLS
  Mat3 R = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
  double mu = 1, prev_cost = inf;
  int iter = 0;
  for (; iter < G.max_iterations; ++iter)
  {
    double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kFinPerLane; ++k)
    {
      const int i = tid + k * kBlock;
      if (i < n)
      {
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
          const double xw = s_ts[r * SAGE_REG_MAX_POINTS + i] * w[k];
#pragma unroll
          for (int c = 0; c < 3; ++c)
            h[3 * r + c] += xw * s_td[c * SAGE_REG_MAX_POINTS + i];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q)
    {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)
        h[q] += __shfl_down(h[q], o, 64);
      if (lane == 0)
        L.H[wave][q] = h[q];
    }
    __syncthreads();
    Mat3 H;
#pragma unroll
    for (int q = 0; q < 9; ++q)
    {
      double s = L.H[0][q];
#pragma unroll
      for (int v = 1; v < kWaves; ++v)
        s += L.H[v][q];
      H.m[q / 3][q % 3] = s;
    }
    R = sage_reg::svd_rot_of(H);

    double rsq[kFinPerLane], part = 0.0, largest = -inf;
#pragma unroll
    for (int k = 0; k < kFinPerLane; ++k)
    {
      const int i = tid + k * kBlock;
      rsq[k] = 0.0;
      if (i < n)
      {
        const double x0 = s_ts[i], x1 = s_ts[SAGE_REG_MAX_POINTS + i], x2 = s_ts[2 * SAGE_REG_MAX_POINTS + i];
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
          const double d = s_td[r * SAGE_REG_MAX_POINTS + i] - (R.m[r][0] * x0 + R.m[r][1] * x1 + R.m[r][2] * x2);
          s += d * d;
        }
        rsq[k] = s;
        part += w[k] * s;
        largest = fmax(largest, s);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
      part += __shfl_down(part, o, 64);
      largest = fmax(largest, __shfl_down(largest, o, 64));
    }
    if (lane == 0)
    {
      L.cost[wave][0] = part;
      L.cost[wave][1] = largest;
    }
    __syncthreads();
    double cost = L.cost[0][0], max_residual = L.cost[0][1];
#pragma unroll
    for (int v = 1; v < kWaves; ++v)
    {
      cost += L.cost[v][0];
      max_residual = fmax(max_residual, L.cost[v][1]);
    }
    if (iter == 0)
    {
      mu = 1 / (2 * max_residual / noise_bound_sq - 1);
      if (mu <= 0)
        break;
    }
#pragma unroll
    for (int k = 0; k < kFinPerLane; ++k)
    {
      const double th1 = (mu + 1) / mu * bsq[k], th2 = mu / (mu + 1) * bsq[k];
      if (tid + k * kBlock < n)
      {
        if (rsq[k] >= th1)
          w[k] = 0;
        else if (rsq[k] <= th2)
          w[k] = 1;
        else
          w[k] = sqrt(bsq[k] * mu * (mu + 1) / rsq[k]) - mu;
      }
    }
    const double cost_diff = fabs(cost - prev_cost);
    mu = mu * G.gnc_factor;
    prev_cost = cost;
    if (cost_diff < G.cost_threshold)
      break;
  }

  int32_t *list = reinterpret_cast<int32_t *>(it.out + 1);
  uint8_t *rotation_mask = reinterpret_cast<uint8_t *>(list + n);
  int n_rot = 0;
#pragma unroll
  for (int k = 0; k < kFinPerLane; ++k)
  {
    const int i = tid + k * kBlock;
    const bool in = i < n && w[k] >= 0.5;
    if (i < n)
      rotation_mask[i] = in ? 1 : 0;
    if (k * kBlock < n) // (uniform)
      n_rot += reg_block_count(in, L.cnt);
  }

  // ---- the translation: three scalar votes over the TIMs' LDS
  __syncthreads();
  uint64_t *s_k = reinterpret_cast<uint64_t *>(L.tim);
  double2 *s_xr = reinterpret_cast<double2 *>(L.tim + kFinEnds);
  uint32_t *s_p = reinterpret_cast<uint32_t *>(L.tim + 2 * kFinEnds);
  int P2 = 4;
  while (P2 < 2 * n)
    P2 <<= 1;
  const int per = P2 > kBlock ? P2 / kBlock : 1; // consecutive sorted endpoints per lane of the scan
  double alpha[kFinPerLane], raw[kFinPerLane], t[3];
  bool mask[kFinPerLane];
#pragma unroll
  for (int k = 0; k < kFinPerLane; ++k)
  {
    const int i = tid + k * kBlock;
    mask[k] = i < n;
    alpha[k] = i < n ? (double)nbf[i] * G.sqrt_cbar2 : 0.0;
  }
  for (int r = 0; r < 3; ++r)
  {
    const double sR0 = scale * R.m[r][0], sR1 = scale * R.m[r][1], sR2 = scale * R.m[r][2];
#pragma unroll
    for (int k = 0; k < kFinPerLane; ++k)
    {
      const int i = tid + k * kBlock;
      raw[k] = 0.0;
      if (i < n)
      {
        raw[k] = (double)dst[3 * i + r] - (sR0 * (double)src[3 * i + 0] + sR1 * (double)src[3 * i + 1] + sR2 * (double)src[3 * i + 2]);
        s_xr[i] = make_double2(raw[k], alpha[k]);
        s_k[2 * i] = reg_key(raw[k] - alpha[k]);
        s_p[2 * i] = 2u * (uint32_t)i;
        s_k[2 * i + 1] = reg_key(raw[k] + alpha[k]);
        s_p[2 * i + 1] = 2u * (uint32_t)i + 1u;
      }
    }
    for (int q = 2 * n + tid; q < P2; q += kBlock)
    {
      s_k[q] = kRegPadKey;
      s_p[q] = kRegPadPayload;
    }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1)
      {
        for (int x = tid; x < P2 / 2; x += kBlock)
        {
          const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
          const bool up = (lo & k) == 0;
          const uint64_t ka = s_k[lo], kb = s_k[hi];
          const uint32_t pa = s_p[lo], pb = s_p[hi];
          if (reg_after(ka, pa, kb, pb) == up)
          {
            s_k[lo] = kb;
            s_k[hi] = ka;
            s_p[lo] = pb;
            s_p[hi] = pa;
          }
        }
        __syncthreads();
      }
    // the running sums, the cost at every endpoint, the first smallest (reg_cost_body on one tile)
    const int at = tid * per;
    uint32_t pl[kRegPerLane];
    double v[kRegQ] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < kRegPerLane; ++e)
    {
      pl[e] = (e < per && at + e < P2) ? s_p[at + e] : kRegPadPayload;
      double q[kRegQ];
      reg_term(pl[e], s_xr, q);
#pragma unroll
      for (int c = 0; c < kRegQ; ++c)
        v[c] += q[c];
    }
    double run[kRegQ], total[kRegQ];
    reg_block_scan(v, run, total, L.wave);
    const double r_all = total[5];
    RegMin best;
    best.cost = inf;
    best.x = 0.0;
    best.idx = kRegNoIndex;
#pragma unroll
    for (int e = 0; e < kRegPerLane; ++e)
    {
      double q[kRegQ];
      reg_term(pl[e], s_xr, q);
#pragma unroll
      for (int c = 0; c < kRegQ; ++c)
        run[c] += q[c];
      if (pl[e] != kRegPadPayload)
      {
        const double x = run[1] / run[0];
        const double residual = (run[6] * x) * x + run[4] - (2.0 * run[3]) * x;
        const double cost = residual + (r_all - run[2]);
        if (cost < best.cost) // (false for a NaN; the first of equal costs stays)
        {
          best.cost = cost;
          best.x = x;
          best.idx = at + e;
        }
      }
    }
    best = reg_block_min(best, L.min);
    t[r] = best.idx != kRegNoIndex ? best.x : __longlong_as_double(0x7ff8000000000000ll); // (no cost but NaNs: the host's NaN)
#pragma unroll
    for (int k = 0; k < kFinPerLane; ++k)
      mask[k] = mask[k] && fabs(raw[k] - t[r]) <= alpha[k];
  }

  // ---- the inlier list, ascending
  int total_in = 0; // the same in every thread
#pragma unroll
  for (int k = 0; k < kFinPerLane; ++k)
  {
    if (k * kBlock >= n) // (uniform)
      continue;
    const int i = tid + k * kBlock;
    const bool keep = mask[k];
    int inc = keep ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o)
        inc += up;
    }
    if (lane == 63)
      L.cnt[wave] = inc;
    __syncthreads();
    int before = total_in, tile = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v)
    {
      if (v < wave)
        before += L.cnt[v];
      tile += L.cnt[v];
    }
    if (keep)
    {
      const int m = before + inc - 1;
      list[m] = i;
      if (it.inliers_dev)
        it.inliers_dev[m] = it.map ? it.map[i] : i;
    }
    total_in += tile;
    __syncthreads(); // (L.cnt is written again)
  }
  if (tid == 0)
  {
#pragma unroll
    for (int q = 0; q < 9; ++q)
      it.out->R[q] = R.m[q / 3][q % 3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
      it.out->t[q] = t[q];
    it.out->valid = 1;
    it.out->n_inliers = total_in;
    it.out->rotation_iterations = iter;
    it.out->n_rotation_inliers = n_rot;
  }
}

// grid: the voting problems.  ticket NULL: it comes behind this launch in the stream (ws_ticket_wait); else one workgroup,
// which posts it itself
__global__ __launch_bounds__(kBlock) void reg_finish_kernel(const RegFinishBatch G, volatile unsigned *ticket, unsigned epoch)
{
  __shared__ RegFinishLds L;
  reg_finish_body(G.item[blockIdx.x], G, L);
  __threadfence_system();
  if (!ticket)
    return;
  __syncthreads(); // (every lane arrives: the body's early return is the whole workgroup's)
  if (threadIdx.x == 0)
  {
    __threadfence_system();
    *ticket = epoch;
  }
}
} // namespace

// a problem's published record -> its result (zeroed by the caller): the counts, then, if the vote was not empty, the host
// finish, which leaves the translation inliers behind the points in the record
static int reg_finish_record(RegHost *h, int N, const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host)
{
  res->n_pairs = h->n_pairs;
  res->n_degenerate_pairs = h->n_degenerate;
  if (!h->vote_valid)
    return SAGE_OK; // (valid = 0: no pair was left in the vote)
  const double scale = h->scale, scale_cost = h->scale_cost;
  const int n_pairs = h->n_pairs, n_scale_inliers = h->n_scale_inliers, n_degenerate = h->n_degenerate;
  int32_t *inl = reinterpret_cast<int32_t *>(h->pts + 7 * (size_t)N);
  if (int rc = sage_registration_finish(h->pts, h->pts + 3 * (size_t)N, h->pts + 6 * (size_t)N, N, scale, p, res, inl, nullptr))
    return rc;
  res->n_pairs = n_pairs;
  res->n_degenerate_pairs = n_degenerate;
  res->n_scale_inlier_pairs = n_scale_inliers;
  res->scale_cost = scale_cost;
  if (inliers_host)
    std::memcpy(inliers_host, inl, (size_t)res->n_inliers * sizeof(int32_t));
  return SAGE_OK;
}

// what a vote leaves to a finish kernel that follows it in the stream (SAGE_REG_FINISH_DEVICE).  Given to a vote, the vote
// reserves extra_pinned bytes behind its own records, does not wait, and says where each segment's tile minima are
struct RegVoteTail
{
  size_t extra_pinned;
  const RegTileMin *tile_min[SAGE_REG_MAX_BATCH];
  int n_tiles[SAGE_REG_MAX_BATCH];
};

// SAGE_REG_FINISH_DEVICE (below): a plan's votes, reg_finish_kernel behind them, one wait, the results out of the records
static int registration_device(SageWorkspace *ws, const RegBatchPlan &plan, const SageRegistrationProblem *probs,
                               const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host, int inliers_stride,
                               const int32_t *const *inlier_map, int *launches_out);

// one problem's vote (N >= 2): reserve, launch, wait for the ticket the publish kernel posts; the record is then at the
// start of ws->reg_host.  *launches (may be NULL): how many kernels that took.  tail (may be NULL): above
static int reg_vote_single(SageWorkspace *ws, const float *src_dev, const float *dst_dev, const float *noise_bounds_dev, int N, double cbar2,
                           int *launches, RegVoteTail *tail = nullptr)
{
  int rc;
  const int n_pairs = N * (N - 1) / 2;
  const int tile = registration_sort_tile(); // (SAGE_REG_SORT_TILE picks another: scripts/registration_bench.py times the three sizes)
  const auto sort_tile = tile == 1024 ? reg_sort_tile_kernel<1024> : tile == 2048 ? reg_sort_tile_kernel<2048> : reg_sort_tile_kernel<4096>;
  int P = kSortTileMax; // (whatever the tile: the workspace's sizes do not depend on the measurement switch)
  while (P < 2 * n_pairs)
    P <<= 1;
  const int n_tiles = (2 * n_pairs + kRegTile - 1) / kRegTile; // tiles that hold an endpoint (the padding sorts behind them)
  // reg_tiles: [n_tiles] sums | [n_tiles + 1] offsets | [n_tiles] minima | counters
  const size_t sums_bytes = (size_t)n_tiles * kRegRow * sizeof(double), offs_bytes = (size_t)(n_tiles + 1) * kRegRow * sizeof(double),
               min_bytes = (size_t)n_tiles * sizeof(RegTileMin);
  if ((rc = ws->reg_keys.reserve((size_t)P * sizeof(uint64_t))) || (rc = ws->reg_payload.reserve((size_t)P * sizeof(uint32_t))) ||
      (rc = ws->reg_pairs.reserve((size_t)n_pairs * sizeof(double2))) ||
      (rc = ws->reg_tiles.reserve(sums_bytes + offs_bytes + min_bytes + 4 * sizeof(int))) ||
      (rc = ws->reg_host.reserve(offsetof(RegHost, pts) + (size_t)N * (7 * sizeof(float) + sizeof(int32_t)) +
                                 (tail ? tail->extra_pinned : 0)))) // (every earlier call has been waited for)
    return rc;
  uint64_t *keys = ws->reg_keys.as<uint64_t>();
  uint32_t *payload = ws->reg_payload.as<uint32_t>();
  double2 *pairs = ws->reg_pairs.as<double2>();
  char *tiles = ws->reg_tiles.as<char>();
  double *tile_sums = reinterpret_cast<double *>(tiles);
  double *tile_offs = reinterpret_cast<double *>(tiles + sums_bytes);
  RegTileMin *tile_min = reinterpret_cast<RegTileMin *>(tiles + sums_bytes + offs_bytes);
  int *counters = reinterpret_cast<int *>(tiles + sums_bytes + offs_bytes + min_bytes);
  RegHost *h = ws->reg_host.as<RegHost>();
  hipStream_t s = ws->stream;

  SAGE_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(int), s));
  const int half_P = P / 2, half_blocks = (half_P + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(reg_pair_kernel, dim3(half_blocks), dim3(kBlock), 0, s, src_dev, dst_dev, noise_bounds_dev, N, n_pairs, half_P,
                     std::sqrt(cbar2), keys, payload, pairs, counters);
  hipLaunchKernelGGL(sort_tile, dim3(P / tile), dim3(kBlock), 0, s, keys, payload, 2, tile);
  const int quarter_P = P / 4, quarter_blocks = (quarter_P + kBlock - 1) / kBlock;
  for (int k = 2 * tile; k <= P; k <<= 1)
  {
    // the distances k / 2 .. tile across tiles: an odd one out first, then two per launch; the rest on the tiles in LDS
    int j = k >> 1, n_global = 0;
    for (int q = j; q >= tile; q >>= 1)
      ++n_global;
    if (n_global & 1)
    {
      hipLaunchKernelGGL(reg_sort_stage_kernel, dim3(half_blocks), dim3(kBlock), 0, s, keys, payload, k, j, half_P);
      j >>= 1;
    }
    for (; j >= 2 * tile; j >>= 2)
      hipLaunchKernelGGL(reg_sort_stage2_kernel, dim3(quarter_blocks), dim3(kBlock), 0, s, keys, payload, k, j, quarter_P);
    hipLaunchKernelGGL(sort_tile, dim3(P / tile), dim3(kBlock), 0, s, keys, payload, k, k);
  }
  hipLaunchKernelGGL(reg_tile_sums_kernel, dim3(n_tiles), dim3(kBlock), 0, s, payload, pairs, tile_sums);
  hipLaunchKernelGGL(reg_tile_offsets_kernel, dim3(1), dim3(kBlock), 0, s, tile_sums, tile_offs, n_tiles);
  hipLaunchKernelGGL(reg_cost_kernel, dim3(n_tiles), dim3(kBlock), 0, s, payload, pairs, tile_offs, n_tiles, tile_min);
  hipLaunchKernelGGL(reg_count_kernel, dim3((n_pairs + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pairs, n_pairs, tile_min, n_tiles,
                     counters);
  const unsigned epoch = ws_ticket_next(ws);
  hipLaunchKernelGGL(reg_publish_kernel, dim3(1), dim3(kBlock), 0, s, src_dev, dst_dev, noise_bounds_dev, N, n_pairs, tile_min, n_tiles,
                     counters, h, &ws->hs()->ticket, epoch);
  SAGE_HIP(hipGetLastError());
  if (launches)
    *launches = registration_sort_launches(P, tile) + kRegSingleFixedLaunches;
  if (tail) // (the publish kernel's ticket is nobody's: the finish kernel posts the one that is awaited)
  {
    tail->tile_min[0] = tile_min;
    tail->n_tiles[0] = n_tiles;
    return SAGE_OK;
  }
  return ws_ticket_await(ws, epoch);
}

extern "C" int sage_robust_registration(SageWorkspace *ws, const float *src_dev, const float *dst_dev, const float *noise_bounds_dev,
                                        int N, const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host,
                                        int32_t *inliers_dev)
{
  if (!ws || !src_dev || !dst_dev || !noise_bounds_dev || !p || !res || N < 0 || N > SAGE_REG_MAX_POINTS)
    return SAGE_E_INVALID;
  int rc;
  if ((rc = registration_check_params(p)))
    return rc;
  if (ws->reg_finish_mode == SAGE_REG_FINISH_DEVICE && p->rotation_max_iterations > SAGE_REG_FINISH_MAX_ITERATIONS)
    return SAGE_E_UNSUPPORTED; // (the kernel's loops are bounded)
  std::memset(res, 0, sizeof(*res));
  if (N < 2)
    return SAGE_OK; // (valid = 0: the reference never calls the solver there)
  if (ws->reg_finish_mode == SAGE_REG_FINISH_DEVICE) // (a batch of one: the batch's contract holds by construction)
  {
    SageRegistrationProblem q{src_dev, dst_dev, noise_bounds_dev, N, p->noise_bound, inliers_dev};
    const int32_t one = N;
    RegBatchPlan plan;
    registration_batch_plan(&one, 1, registration_sort_tile(), &plan);
    int launches;
    return registration_device(ws, plan, &q, p, res, inliers_host, N, nullptr, &launches);
  }
  if ((rc = reg_vote_single(ws, src_dev, dst_dev, noise_bounds_dev, N, p->cbar2, nullptr)))
    return rc;
  RegHost *h = ws->reg_host.as<RegHost>();
  hipStream_t s = ws->stream;
  if ((rc = reg_finish_record(h, N, p, res, inliers_host)))
    return rc;
  if (inliers_dev && res->n_inliers > 0)
  {
    const int32_t *inl = reinterpret_cast<const int32_t *>(h->pts + 7 * (size_t)N); // (pinned: the source of the copy)
    SAGE_HIP(hipMemcpyAsync(inliers_dev, inl, (size_t)res->n_inliers * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if ((rc = ws_ticket_wait(ws)))
      return rc;
  }
  return SAGE_OK;
}

// the votes of a plan's segments (two or more): reserve, launch, one ticket behind the publish launch, wait.  record [plan.n]:
// where each segment's pinned record is
static int reg_vote_batch(SageWorkspace *ws, const RegBatchPlan &plan, const SageRegistrationProblem *probs, double cbar2,
                          RegHost **record, int *launches_out, RegVoteTail *tail = nullptr)
{
  int rc;
  if ((rc = ws->reg_keys.reserve((size_t)plan.keys_bytes)) || (rc = ws->reg_payload.reserve((size_t)plan.payload_bytes)) ||
      (rc = ws->reg_pairs.reserve((size_t)plan.pairs_bytes)) || (rc = ws->reg_tiles.reserve((size_t)plan.tiles_bytes)) ||
      (rc = ws->reg_host.reserve((size_t)plan.pinned_bytes + (tail ? tail->extra_pinned : 0)))) // (every earlier call has been waited for)
    return rc;
  uint64_t *keys = ws->reg_keys.as<uint64_t>();
  uint32_t *payload = ws->reg_payload.as<uint32_t>();
  double2 *pairs = ws->reg_pairs.as<double2>();
  char *tiles = ws->reg_tiles.as<char>();
  char *records = ws->reg_host.as<char>();
  hipStream_t s = ws->stream;

  RegSegTable T{};
  RegSegPoints Q{};
  T.n = plan.n;
  for (int i = 0; i < plan.n; ++i)
  {
    const RegBatchSegment &g = plan.seg[i];
    T.start[i] = g.start; T.tile0[i] = g.tile0; T.cblock0[i] = g.cblock0; T.pair0[i] = g.pair0;
    T.N[i] = g.N; T.n_pairs[i] = g.pairs; T.n_tiles[i] = g.n_tiles; T.rows0[i] = g.rows0;
    Q.src[i] = probs[g.row].src_dev; Q.dst[i] = probs[g.row].dst_dev; Q.nb[i] = probs[g.row].noise_bounds_dev;
    Q.host[i] = reinterpret_cast<RegHost *>(records + g.record0);
  }
  T.start[plan.n] = plan.endpoints; T.tile0[plan.n] = plan.tiles; T.cblock0[plan.n] = plan.cblocks;

  int launches = 0;
  const int tile = plan.sort_tile;
  const auto sort_tile = tile == 1024   ? reg_sort_tile_batch_kernel<1024>
                         : tile == 2048 ? reg_sort_tile_batch_kernel<2048>
                                        : reg_sort_tile_batch_kernel<4096>;
  SAGE_HIP(hipMemsetAsync(tiles, 0, 16 * (size_t)plan.n, s)); // the segments' counters
  hipLaunchKernelGGL(reg_pair_batch_kernel, dim3(plan.endpoints / (2 * kBlock)), dim3(kBlock), 0, s, T, Q, std::sqrt(cbar2), keys, payload,
                     pairs, tiles);
  hipLaunchKernelGGL(sort_tile, dim3(plan.endpoints / tile), dim3(kBlock), 0, s, T, keys, payload, 2, tile);
  launches += 2;
  int n_k = plan.n; // the segments a stage with k concerns: those with P >= k, the first n_k
  for (int k = 2 * tile; k <= plan.seg[0].P; k <<= 1)
  {
    while (plan.seg[n_k - 1].P < k)
      --n_k;
    const int ends = plan.seg[n_k - 1].start + plan.seg[n_k - 1].P; // (a multiple of 4096)
    // the distances k / 2 .. tile across tiles: an odd one out first, then two per launch; the rest on the tiles in LDS
    int j = k >> 1, n_global = 0;
    for (int q = j; q >= tile; q >>= 1)
      ++n_global;
    if (n_global & 1)
    {
      hipLaunchKernelGGL(reg_sort_stage_batch_kernel, dim3(ends / (2 * kBlock)), dim3(kBlock), 0, s, T, keys, payload, k, j);
      ++launches;
      j >>= 1;
    }
    for (; j >= 2 * tile; j >>= 2, ++launches)
      hipLaunchKernelGGL(reg_sort_stage2_batch_kernel, dim3(ends / (4 * kBlock)), dim3(kBlock), 0, s, T, keys, payload, k, j);
    hipLaunchKernelGGL(sort_tile, dim3(ends / tile), dim3(kBlock), 0, s, T, keys, payload, k, k);
    ++launches;
  }
  hipLaunchKernelGGL(reg_tile_sums_batch_kernel, dim3(plan.tiles), dim3(kBlock), 0, s, T, payload, pairs, tiles);
  hipLaunchKernelGGL(reg_tile_offsets_batch_kernel, dim3(plan.n), dim3(kBlock), 0, s, T, tiles);
  hipLaunchKernelGGL(reg_cost_batch_kernel, dim3(plan.tiles), dim3(kBlock), 0, s, T, payload, pairs, tiles);
  hipLaunchKernelGGL(reg_count_batch_kernel, dim3(plan.cblocks), dim3(kBlock), 0, s, T, pairs, tiles);
  hipLaunchKernelGGL(reg_publish_batch_kernel, dim3(plan.n), dim3(kBlock), 0, s, T, Q, tiles);
  SAGE_HIP(hipGetLastError());
  launches += 5 + 1; // (and the ticket's)
  *launches_out = launches;
  for (int i = 0; i < plan.n; ++i)
    record[i] = Q.host[i];
  if (tail) // (the ticket, counted above, comes behind the finish kernel)
  {
    for (int i = 0; i < plan.n; ++i)
    {
      // (reg_segment_rows: [n_tiles] sums | [n_tiles + 1] offsets | [n_tiles] minima)
      tail->tile_min[i] = reinterpret_cast<const RegTileMin *>(tiles + plan.seg[i].rows0 +
                                                               (2 * (size_t)plan.seg[i].n_tiles + 1) * kRegRow * sizeof(double));
      tail->n_tiles[i] = plan.seg[i].n_tiles;
    }
    return SAGE_OK;
  }
  return ws_ticket_wait(ws);
}

// the finish kernel over n items: one launch and the ticket's, or (own_ticket: one workgroup) one launch that posts it; waits
static int reg_finish_launch(SageWorkspace *ws, const RegFinishBatch &G, int n, bool own_ticket)
{
  if (own_ticket)
  {
    const unsigned epoch = ws_ticket_next(ws);
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(kBlock), 0, ws->stream, G, &ws->hs()->ticket, epoch);
    SAGE_HIP(hipGetLastError());
    return ws_ticket_await(ws, epoch);
  }
  hipLaunchKernelGGL(reg_finish_kernel, dim3(n), dim3(kBlock), 0, ws->stream, G, (volatile unsigned *)nullptr, 0u);
  SAGE_HIP(hipGetLastError());
  return ws_ticket_wait(ws);
}

static void reg_finish_params(const SageRegistrationParams *p, RegFinishBatch *G)
{
  G->sqrt_cbar2 = std::sqrt(p->cbar2);
  G->cost_threshold = p->rotation_cost_threshold;
  G->gnc_factor = p->rotation_gnc_factor;
  G->max_iterations = p->rotation_max_iterations;
}

// a finish record -> the finish's fields of a result (zeroed by the caller), the list and the rotation mask
static void reg_finish_read(const RegFinishHost *f, int N, SageRegistrationResult *res, int32_t *inliers_host, uint8_t *rotation_mask)
{
  res->valid = f->valid;
  if (!f->valid)
    return;
  std::memcpy(res->R, f->R, sizeof(res->R));
  std::memcpy(res->t, f->t, sizeof(res->t));
  res->n_inliers = f->n_inliers;
  res->rotation_iterations = f->rotation_iterations;
  res->n_rotation_inliers = f->n_rotation_inliers;
  const int32_t *list = reinterpret_cast<const int32_t *>(f + 1);
  if (inliers_host)
    std::memcpy(inliers_host, list, (size_t)f->n_inliers * sizeof(int32_t));
  if (rotation_mask)
    std::memcpy(rotation_mask, list + N, (size_t)N);
}

static int registration_device(SageWorkspace *ws, const RegBatchPlan &plan, const SageRegistrationProblem *probs,
                               const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host, int inliers_stride,
                               const int32_t *const *inlier_map, int *launches_out)
{
  int rc, launches = 0;
  RegVoteTail tail{};
  size_t off[SAGE_REG_MAX_BATCH];
  for (int i = 0; i < plan.n; ++i)
  {
    off[i] = tail.extra_pinned;
    tail.extra_pinned += (size_t)reg_finish_record_bytes(plan.seg[i].N);
  }
  RegHost *seg_record[SAGE_REG_MAX_BATCH];
  if (plan.n == 1)
  {
    const SageRegistrationProblem &q = probs[plan.seg[0].row];
    rc = reg_vote_single(ws, q.src_dev, q.dst_dev, q.noise_bounds_dev, q.N, p->cbar2, &launches, &tail);
    seg_record[0] = ws->reg_host.as<RegHost>();
  }
  else
    rc = reg_vote_batch(ws, plan, probs, p->cbar2, seg_record, &launches, &tail);
  if (rc)
    return rc;
  char *fin = ws->reg_host.as<char>() + plan.pinned_bytes; // (the finish records: behind the votes')
  RegFinishBatch G{};
  reg_finish_params(p, &G);
  for (int i = 0; i < plan.n; ++i)
  {
    const int b = plan.seg[i].row;
    RegFinishItem &it = G.item[i];
    it.src = probs[b].src_dev; it.dst = probs[b].dst_dev; it.nb = probs[b].noise_bounds_dev;
    it.tile_min = tail.tile_min[i]; it.n_tiles = tail.n_tiles[i];
    it.out = reinterpret_cast<RegFinishHost *>(fin + off[i]);
    it.inliers_dev = probs[b].inliers_dev;
    it.map = inlier_map ? inlier_map[b] : nullptr;
    it.noise_bound = probs[b].noise_bound;
    it.N = probs[b].N;
  }
  if ((rc = reg_finish_launch(ws, G, plan.n, plan.n == 1)))
    return rc;
  *launches_out = launches + 1;
  for (int i = 0; i < plan.n; ++i)
  {
    const int b = plan.seg[i].row;
    const RegHost *h = seg_record[i];
    res[b].n_pairs = h->n_pairs;
    res[b].n_degenerate_pairs = h->n_degenerate;
    if (!h->vote_valid)
      continue; // (valid = 0: no pair was left in the vote)
    reg_finish_read(G.item[i].out, probs[b].N, &res[b], inliers_host ? inliers_host + (size_t)b * inliers_stride : nullptr, nullptr);
    res[b].scale = h->scale;
    res[b].n_scale_inlier_pairs = h->n_scale_inliers;
    res[b].scale_cost = h->scale_cost;
  }
  return SAGE_OK;
}

// the batch: plan, reserve, launch, wait once, finish per problem in row order, then the inliers_dev rows in one launch.
// inlier_map (NULL, or [B] device arrays): row b of inliers_dev receives inlier_map[b][inlier] instead of the inlier (the
// pre-check's keypoint positions)
static int registration_batch(SageWorkspace *ws, const SageRegistrationProblem *probs, int B, const SageRegistrationParams *p,
                              SageRegistrationResult *res, int32_t *inliers_host, int inliers_stride, const int32_t *const *inlier_map)
{
  if (B < 0 || B > SAGE_REG_MAX_BATCH)
    return SAGE_E_INVALID;
  if (B == 0)
    return SAGE_OK;
  if (!ws || !probs || !p || !res)
    return SAGE_E_INVALID;
  int rc;
  SageRegistrationParams pp = *p;
  pp.noise_bound = 1.0; // (replaced per problem below: the caller's value is not read)
  if ((rc = registration_check_params(&pp)))
    return rc;
  const bool device = ws->reg_finish_mode == SAGE_REG_FINISH_DEVICE;
  if (device && p->rotation_max_iterations > SAGE_REG_FINISH_MAX_ITERATIONS)
    return SAGE_E_UNSUPPORTED; // (the kernel's loops are bounded)
  int32_t Ns[SAGE_REG_MAX_BATCH];
  int max_N = 0;
  for (int b = 0; b < B; ++b)
  {
    const SageRegistrationProblem &q = probs[b];
    if (q.N < 0 || q.N > SAGE_REG_MAX_POINTS)
      return SAGE_E_INVALID;
    if (q.N >= 2 && (!q.src_dev || !q.dst_dev || !q.noise_bounds_dev || !(q.noise_bound > 0) || !std::isfinite(q.noise_bound)))
      return SAGE_E_INVALID;
    Ns[b] = q.N;
    max_N = std::max(max_N, (int)q.N);
  }
  if (inliers_host && inliers_stride < max_N)
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
    std::memset(&res[b], 0, sizeof(res[b]));
  ws->reg_batch_launches = 0;

  RegBatchPlan plan;
  registration_batch_plan(Ns, B, registration_sort_tile(), &plan);
  if (plan.n == 0)
    return SAGE_OK; // (nothing votes: valid = 0 everywhere, no launch)
  if (device)
    return registration_device(ws, plan, probs, p, res, inliers_host, inliers_stride, inlier_map, &ws->reg_batch_launches);
  // a batch with ONE voting problem takes the single call's path (its publish kernel posts the ticket itself: one launch
  // fewer, and the batch of one is then no slower than the call it replaces -- measured: scripts/registration_batch_bench.py)
  RegHost *seg_record[SAGE_REG_MAX_BATCH];
  if (plan.n == 1)
  {
    const SageRegistrationProblem &q = probs[plan.seg[0].row];
    rc = reg_vote_single(ws, q.src_dev, q.dst_dev, q.noise_bounds_dev, q.N, p->cbar2, &ws->reg_batch_launches);
    seg_record[0] = ws->reg_host.as<RegHost>();
  }
  else
    rc = reg_vote_batch(ws, plan, probs, p->cbar2, seg_record, &ws->reg_batch_launches);
  if (rc)
    return rc;
  hipStream_t s = ws->stream;

  RegHost *record[SAGE_REG_MAX_BATCH] = {};
  for (int i = 0; i < plan.n; ++i)
    record[plan.seg[i].row] = seg_record[i];
  RegRowCopy rows{};
  int n_rows = 0, max_n = 0;
  for (int b = 0; b < B; ++b)
  {
    if (!record[b])
      continue;
    pp.noise_bound = probs[b].noise_bound;
    if ((rc = reg_finish_record(record[b], probs[b].N, &pp, &res[b], inliers_host ? inliers_host + (size_t)b * inliers_stride : nullptr)))
      return rc;
    if (probs[b].inliers_dev && res[b].n_inliers > 0)
    {
      rows.in[n_rows] = reinterpret_cast<const int32_t *>(record[b]->pts + 7 * (size_t)probs[b].N);
      rows.map[n_rows] = inlier_map ? inlier_map[b] : nullptr;
      rows.out[n_rows] = probs[b].inliers_dev;
      rows.n[n_rows] = res[b].n_inliers;
      max_n = std::max(max_n, res[b].n_inliers);
      ++n_rows;
    }
  }
  if (n_rows)
  {
    hipLaunchKernelGGL(reg_row_copy_kernel, dim3((max_n + kBlock - 1) / kBlock, n_rows), dim3(kBlock), 0, s, rows);
    SAGE_HIP(hipGetLastError());
    ws->reg_batch_launches += 2;
    if ((rc = ws_ticket_wait(ws)))
      return rc;
  }
  return SAGE_OK;
}

extern "C" int sage_robust_registration_batch(SageWorkspace *ws, const SageRegistrationProblem *probs, int B,
                                              const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host,
                                              int inliers_stride)
{
  return registration_batch(ws, probs, B, p, res, inliers_host, inliers_stride, nullptr);
}

extern "C" int sage_robust_registration_batch_launches(const SageWorkspace *ws) { return ws ? ws->reg_batch_launches : 0; }

extern "C" int sage_workspace_set_registration_finish(SageWorkspace *ws, int mode)
{
  if (!ws || (mode != SAGE_REG_FINISH_HOST && mode != SAGE_REG_FINISH_DEVICE))
    return SAGE_E_INVALID;
  ws->reg_finish_mode = mode;
  return SAGE_OK;
}

extern "C" int sage_workspace_registration_finish(const SageWorkspace *ws) { return ws ? ws->reg_finish_mode : SAGE_REG_FINISH_HOST; }

extern "C" int sage_registration_finish_batch(SageWorkspace *ws, const SageRegistrationProblem *probs, int B, const double *scales,
                                              const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host,
                                              int inliers_stride, uint8_t *rotation_masks)
{
  if (B < 0 || B > SAGE_REG_MAX_BATCH)
    return SAGE_E_INVALID;
  if (B == 0)
    return SAGE_OK;
  if (!ws || !probs || !scales || !p || !res)
    return SAGE_E_INVALID;
  int rc;
  SageRegistrationParams pp = *p;
  pp.noise_bound = 1.0; // (replaced per problem: the caller's value is not read)
  if ((rc = registration_check_params(&pp)))
    return rc;
  if (p->rotation_max_iterations > SAGE_REG_FINISH_MAX_ITERATIONS)
    return SAGE_E_UNSUPPORTED; // (the kernel's loops are bounded)
  int max_N = 0;
  for (int b = 0; b < B; ++b)
  {
    const SageRegistrationProblem &q = probs[b];
    if (q.N < 0 || q.N > SAGE_REG_MAX_POINTS)
      return SAGE_E_INVALID;
    if (q.N >= 2 && (!q.src_dev || !q.dst_dev || !q.noise_bounds_dev || !(q.noise_bound > 0) || !std::isfinite(q.noise_bound)))
      return SAGE_E_INVALID;
    max_N = std::max(max_N, (int)q.N);
  }
  if ((inliers_host || rotation_masks) && inliers_stride < max_N)
    return SAGE_E_INVALID;
  RegFinishBatch G{};
  reg_finish_params(p, &G);
  int row[SAGE_REG_MAX_BATCH], n = 0;
  size_t off[SAGE_REG_MAX_BATCH], bytes = 0;
  for (int b = 0; b < B; ++b)
  {
    std::memset(&res[b], 0, sizeof(res[b]));
    if (probs[b].N < 2)
      continue; // (takes no part)
    off[n] = bytes;
    bytes += (size_t)reg_finish_record_bytes(probs[b].N);
    row[n++] = b;
  }
  if (n == 0)
    return SAGE_OK;
  if ((rc = ws->reg_host.reserve(bytes))) // (every earlier call has been waited for)
    return rc;
  char *fin = ws->reg_host.as<char>();
  for (int i = 0; i < n; ++i)
  {
    const int b = row[i];
    RegFinishItem &it = G.item[i];
    it.src = probs[b].src_dev; it.dst = probs[b].dst_dev; it.nb = probs[b].noise_bounds_dev;
    it.out = reinterpret_cast<RegFinishHost *>(fin + off[i]);
    it.inliers_dev = probs[b].inliers_dev;
    it.noise_bound = probs[b].noise_bound;
    it.scale = scales[b];
    it.N = probs[b].N;
  }
  if ((rc = reg_finish_launch(ws, G, n, false)))
    return rc;
  for (int i = 0; i < n; ++i)
  {
    const int b = row[i];
    reg_finish_read(G.item[i].out, probs[b].N, &res[b], inliers_host ? inliers_host + (size_t)b * inliers_stride : nullptr,
                    rotation_masks ? rotation_masks + (size_t)b * inliers_stride : nullptr);
    res[b].scale = scales[b];
  }
  return SAGE_OK;
}

// the scalars of a gather (the pointers are left to the caller)
static MatchPointsParams match_points_scalars(float depth_divisor0, const SageCamera *cam, int K, int W, float noise_multiplier,
                                              int noise_from)
{
  MatchPointsParams P{};
  P.divisor0 = depth_divisor0; P.cx = cam->cx; P.cy = cam->cy; P.fx = cam->fx; P.fy = cam->fy; P.Wf = (float)W;
  P.focal = (float)((cam->fx + cam->fy) / 2.0); // float focal_length = (fx + fy) / 2.0
  P.mult = noise_multiplier;
  P.HW = (long long)cam->w * (long long)cam->h;
  P.K = K; P.noise_from = noise_from;
  return P;
}

extern "C" int sage_match_points(SageWorkspace *ws, const int32_t *cyc_inlier_flags, const int64_t *raw_matched_loc1d_1,
                                 const float *dpts0, const float *homo0, float depth_divisor0, const float *dpt_map_1,
                                 const SageCamera *cam, int K, int W, float noise_multiplier, int noise_from, float *pts0, float *pts1,
                                 float *noise_bounds, float *homo1, float *dpts1, int32_t *kept, int *M_host,
                                 float *mean_noise_depth_host)
{
  if (!ws || !cyc_inlier_flags || !raw_matched_loc1d_1 || !dpts0 || !homo0 || !dpt_map_1 || !cam || !pts0 || !pts1 || !noise_bounds ||
      !homo1 || !dpts1 || !kept || !M_host || K < 1 || W < 1 || !(cam->fx > 0) || !(cam->fy > 0) || !std::isfinite(cam->fx) ||
      !std::isfinite(cam->fy) || (noise_from != 0 && noise_from != 1))
    return SAGE_E_INVALID;
  int rc;
  if ((rc = ws->reg_host.reserve(offsetof(RegHost, pts) + sizeof(float))))
    return rc;
  MatchPointsParams P = match_points_scalars(depth_divisor0, cam, K, W, noise_multiplier, noise_from);
  P.flags = cyc_inlier_flags; P.loc1 = raw_matched_loc1d_1; P.dpts0 = dpts0; P.homo0 = homo0; P.dpt_map_1 = dpt_map_1;
  P.pts0 = pts0; P.pts1 = pts1; P.noise_bounds = noise_bounds; P.homo1 = homo1; P.dpts1 = dpts1; P.kept = kept;
  RegHost *h = ws->reg_host.as<RegHost>();
  const unsigned epoch = ws_ticket_next(ws);
  hipLaunchKernelGGL(reg_match_points_kernel, dim3(1), dim3(kBlock), 0, ws->stream, P, h, &ws->hs()->ticket, epoch);
  SAGE_HIP(hipGetLastError());
  if ((rc = ws_ticket_await(ws, epoch)))
    return rc;
  *M_host = h->M;
  if (mean_noise_depth_host)
    *mean_noise_depth_host = h->mean_depth;
  return SAGE_OK;
}

extern "C" int sage_match_points_batch(SageWorkspace *ws, const SageMatchPointsItem *items, int B, float depth_divisor0,
                                       const SageCamera *cam, int K, int W, float noise_multiplier, int noise_from, int32_t *M_host,
                                       float *mean_noise_depth_host)
{
  if (B < 0 || B > SAGE_REG_MAX_BATCH)
    return SAGE_E_INVALID;
  if (B == 0)
    return SAGE_OK;
  if (!ws || !items || !cam || !M_host || K < 1 || W < 1 || !(cam->fx > 0) || !(cam->fy > 0) || !std::isfinite(cam->fx) ||
      !std::isfinite(cam->fy) || (noise_from != 0 && noise_from != 1))
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
  {
    const SageMatchPointsItem &it = items[b];
    if (!it.cyc_inlier_flags || !it.raw_matched_loc1d_1 || !it.dpts0 || !it.homo0 || !it.dpt_map_1 || !it.pts0 || !it.pts1 ||
        !it.noise_bounds || !it.homo1 || !it.dpts1 || !it.kept)
      return SAGE_E_INVALID;
  }
  if (B == 1) // (the single call's path: its kernel posts the ticket itself, one launch fewer)
    return sage_match_points(ws, items[0].cyc_inlier_flags, items[0].raw_matched_loc1d_1, items[0].dpts0, items[0].homo0, depth_divisor0,
                             items[0].dpt_map_1, cam, K, W, noise_multiplier, noise_from, items[0].pts0, items[0].pts1, items[0].noise_bounds,
                             items[0].homo1, items[0].dpts1, items[0].kept, M_host, mean_noise_depth_host);
  int rc;
  if ((rc = ws->reg_host.reserve(64 * (size_t)B + sizeof(RegHost))))
    return rc;
  MatchPointsBatch G{};
  for (int b = 0; b < B; ++b)
    G.item[b] = items[b];
  G.shared = match_points_scalars(depth_divisor0, cam, K, W, noise_multiplier, noise_from);
  G.host = ws->reg_host.as<RegHost>();
  hipLaunchKernelGGL(reg_match_points_batch_kernel, dim3(B), dim3(kBlock), 0, ws->stream, G);
  SAGE_HIP(hipGetLastError());
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  for (int b = 0; b < B; ++b)
  {
    const RegHost *h = reinterpret_cast<const RegHost *>(ws->reg_host.as<char>() + 64 * (size_t)b);
    M_host[b] = h->M;
    if (mean_noise_depth_host)
      mean_noise_depth_host[b] = h->mean_depth;
  }
  return SAGE_OK;
}

// ---- the loop detector's pre-check: sage_cycle_match_batch, then the two batched calls above over the survivors ----

extern "C" int sage_loop_precheck(SageWorkspace *ws, const float *desc_query_dev, float query_depth_divisor,
                                  const SageLoopCandidate *cands, int B, int K, int C, int H, int W, const SageCamera *cam,
                                  float cyc_thresh, float noise_multiplier, float min_desc_inlier_ratio,
                                  const SageRegistrationParams *p, SageLoopPrecheckResult *results, int64_t *raw_matched_loc1d,
                                  int32_t *inlier_flags, int32_t *inlier_kp_dev)
{
  if (!ws || !cands || !cam || !p || !results || B < 0 || B > SAGE_MATCH_MAX_BATCH || K < 0 || K > SAGE_REG_MAX_POINTS || C < 1 ||
      C > 1024 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffll)
    return SAGE_E_INVALID;
  if (B > 0 && K > 0)
  {
    if (!desc_query_dev || !raw_matched_loc1d || !inlier_flags || !inlier_kp_dev || !(cam->fx > 0) || !(cam->fy > 0) ||
        !std::isfinite(cam->fx) || !std::isfinite(cam->fy))
      return SAGE_E_INVALID;
    for (int b = 0; b < B; ++b)
      if (!cands[b].desc_dev || !cands[b].dpt_map_dev || !cands[b].kp_loc1d_dev || !cands[b].kp_dpts0_dev || !cands[b].kp_homo0_dev)
        return SAGE_E_INVALID;
  }
  int rc;
  SageRegistrationParams pp = *p;
  pp.noise_bound = 1.0; // (replaced per candidate below: the caller's value is not read)
  if ((rc = registration_check_params(&pp)))
    return rc;
  for (int b = 0; b < B; ++b)
    std::memset(&results[b], 0, sizeof(results[b]));
  if (B == 0 || K == 0)
    return SAGE_OK;

  // scratch: the way back [B][K] | per candidate: pts0 [K][3] | pts1 [K][3] | homo1 [K][3] | noise bounds [K] | dpts1 [K] | kept [K]
  const size_t cyc_bytes = (size_t)B * K * sizeof(int64_t), cand_bytes = (size_t)K * (11 * sizeof(float) + sizeof(int32_t));
  if ((rc = ws->pre_scratch.reserve(cyc_bytes + (size_t)B * cand_bytes)))
    return rc;
  int64_t *cyc = ws->pre_scratch.as<int64_t>();
  char *gathered = ws->pre_scratch.as<char>() + cyc_bytes;

  const float *desc[SAGE_MATCH_MAX_BATCH];
  const int64_t *kp[SAGE_MATCH_MAX_BATCH];
  int32_t n_cycle[SAGE_MATCH_MAX_BATCH];
  for (int b = 0; b < B; ++b)
  {
    desc[b] = cands[b].desc_dev;
    kp[b] = cands[b].kp_loc1d_dev;
  }
  if ((rc = sage_cycle_match_batch(ws, desc_query_dev, desc, kp, B, K, C, H, W, cyc_thresh, 0, raw_matched_loc1d, cyc, inlier_flags,
                                   n_cycle)))
    return rc;

  // the gather of every candidate that passes the prune: one launch
  static_assert(SAGE_MATCH_MAX_BATCH <= SAGE_REG_MAX_BATCH, "one batch holds every candidate");
  SageMatchPointsItem items[SAGE_REG_MAX_BATCH];
  int row[SAGE_REG_MAX_BATCH], n_items = 0; // the candidate of an item; later of a problem
  for (int b = 0; b < B; ++b)
  {
    results[b].n_cycle = n_cycle[b];
    // |translation inliers| <= n_cycle: a candidate below the ratio here is below it after the solve as well
    if (n_cycle[b] <= 0 || (float)n_cycle[b] / (float)K < min_desc_inlier_ratio)
      continue;
    float *pts0 = reinterpret_cast<float *>(gathered + (size_t)b * cand_bytes);
    SageMatchPointsItem &it = items[n_items];
    it.cyc_inlier_flags = inlier_flags + (size_t)b * K; it.raw_matched_loc1d_1 = raw_matched_loc1d + (size_t)b * K;
    it.dpts0 = cands[b].kp_dpts0_dev; it.homo0 = cands[b].kp_homo0_dev; it.dpt_map_1 = cands[b].dpt_map_dev;
    it.pts0 = pts0; it.pts1 = pts0 + 3 * (size_t)K; it.homo1 = pts0 + 6 * (size_t)K; it.noise_bounds = pts0 + 9 * (size_t)K;
    it.dpts1 = pts0 + 10 * (size_t)K; it.kept = reinterpret_cast<int32_t *>(pts0 + 11 * (size_t)K);
    row[n_items++] = b;
  }
  int32_t M[SAGE_REG_MAX_BATCH];
  float mean[SAGE_REG_MAX_BATCH];
  if ((rc = sage_match_points_batch(ws, items, n_items, query_depth_divisor, cam, K, W, noise_multiplier, 1, M, mean)))
    return rc;

  // the bound of every candidate that is left, and their solves: one batch
  SageRegistrationProblem probs[SAGE_REG_MAX_BATCH];
  const int32_t *kept[SAGE_REG_MAX_BATCH];
  int n_probs = 0;
  for (int i = 0; i < n_items; ++i)
  {
    SageLoopPrecheckResult &r = results[row[i]];
    r.n_matched = M[i];
    r.mean_noise_depth = mean[i];
    const float nb = (noise_multiplier * r.mean_noise_depth) / ((cam->fx + cam->fy) / 2.0f);
    if (M[i] < 2 || !(nb > 0) || !std::isfinite(nb))
      continue; // (no solve: one match, or depths the bound cannot be made from)
    SageRegistrationProblem &q = probs[n_probs];
    q.src_dev = items[i].pts0; q.dst_dev = items[i].pts1; q.noise_bounds_dev = items[i].noise_bounds;
    q.N = M[i];
    q.noise_bound = (double)nb;
    q.inliers_dev = inlier_kp_dev + (size_t)row[i] * K;
    kept[n_probs] = items[i].kept;
    row[n_probs++] = row[i]; // (n_probs <= i)
  }
  // (each survivor's inlier keypoints kept[inliers] are written from the pinned records in the batch's one copy launch)
  SageRegistrationResult reg[SAGE_REG_MAX_BATCH];
  if ((rc = registration_batch(ws, probs, n_probs, &pp, reg, nullptr, 0, kept)))
    return rc;
  for (int i = 0; i < n_probs; ++i)
  {
    SageLoopPrecheckResult &r = results[row[i]];
    r.reg = reg[i];
    r.registered = 1;
    r.relative_desc_match_inlier_ratio = (float)r.reg.n_inliers / (float)probs[i].N;
    r.desc_match_inlier_ratio = (float)r.reg.n_inliers / (float)K;
  }
  return SAGE_OK;
}

// ---- the loop body after the ratio test: every survivor of the pre-check tracked against the query in one batch ----
namespace
{
struct VerifyGatherItem // one survivor
{
  const float *kp_homo0, *kp_dpts0, *dpt_map;
  const int64_t *raw;      // row b of raw_matched_loc1d
  const int32_t *inlier_kp; // row b of inlier_kp_dev
  float *out;              // row b of kp_gathered_dev: homo0 [K][3] | unscaled dpts0 [K] | homo1 [K][3] | dpts1 [K]
  int32_t n, pad;
};
struct VerifyGatherParams
{
  VerifyGatherItem item[SAGE_TRACK_MAX_BATCH];
  float divisor0, cx, cy, fx, fy, Wf;
  long long HW;
  int K;
};

// grid (ceil(K / 256), survivors): inlier j of survivor blockIdx.y
__global__ __launch_bounds__(kBlock) void verify_gather_kernel(const VerifyGatherParams P)
{
#pragma clang fp contract(off)
  const VerifyGatherItem &it = P.item[blockIdx.y];
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= it.n)
    return;
  const int i = it.inlier_kp[j];
  const size_t K = (size_t)P.K;
  float *homo0 = it.out, *dpts0 = homo0 + 3 * K, *homo1 = dpts0 + K, *dpts1 = homo1 + 3 * K;
  if (i < 0 || i >= P.K) // (not a position among the K keypoints: nothing is read through it, the term turns NaN)
  {
    const float nan = __int_as_float(0x7fc00000);
    homo0[3 * j + 0] = homo0[3 * j + 1] = homo0[3 * j + 2] = dpts0[j] = nan;
    homo1[3 * j + 0] = homo1[3 * j + 1] = homo1[3 * j + 2] = dpts1[j] = nan;
    return;
  }
  homo0[3 * j + 0] = it.kp_homo0[3 * i + 0];
  homo0[3 * j + 1] = it.kp_homo0[3 * i + 1];
  homo0[3 * j + 2] = it.kp_homo0[3 * i + 2];
  dpts0[j] = it.kp_dpts0[i] / P.divisor0;
  float hx, hy, d1;
  matched_point(it.raw[i], P.Wf, P.cx, P.cy, P.fx, P.fy, P.HW, it.dpt_map, &hx, &hy, &d1);
  homo1[3 * j + 0] = hx;
  homo1[3 * j + 1] = hy;
  homo1[3 * j + 2] = 1.0f;
  dpts1[j] = d1;
}
} // namespace

extern "C" int sage_loop_verify(SageWorkspace *ws, const SageLmConfig *cfg, const SageLoopVerifyQuery *query,
                                float query_depth_divisor, const SageLoopCandidate *cands, const SageLoopVerifyCandidate *vcands,
                                const SageLoopPrecheckResult *pre, int B, int K, const int64_t *raw_matched_loc1d,
                                const int32_t *inlier_kp_dev, float match_geom_factor_weight, float *kp_gathered_dev,
                                SageLoopVerifyResult *results)
{
  if (!ws || !cfg || !query || !results || B < 0 || B > SAGE_TRACK_MAX_BATCH || K < 0 || K > SAGE_REG_MAX_POINTS)
    return SAGE_E_INVALID;
  int surv[SAGE_TRACK_MAX_BATCH], ns = 0;
  if (B > 0)
  {
    const SageCamera &cam = query->pyr.cam[0];
    if (!cands || !vcands || !pre || !raw_matched_loc1d || !inlier_kp_dev || !kp_gathered_dev || query->N < 1 || query->M < 1 ||
        (query->FS != 16 && query->FS != 32) || query->pyr.levels < 1 || query->pyr.levels > SAGE_MAX_LEVELS || !query->homo_dev ||
        !query->unscaled_dpts0_dev || !query->feat0s_dev || !query->weights_dev || !query->valid_homo_dev ||
        !query->valid_dpts0_dev || !query->mask_dev || !(cam.fx > 0) || !(cam.fy > 0) || !std::isfinite(cam.fx) ||
        !std::isfinite(cam.fy) || cam.w < 1 || cam.h < 1 || !(query_depth_divisor > 0) || !std::isfinite(query_depth_divisor))
      return SAGE_E_INVALID;
    for (int b = 0; b < B; ++b)
    {
      if (pre[b].registered != 1 || pre[b].reg.n_inliers <= 3) // camera_tracker.cpp:1407
        continue;
      if (pre[b].reg.n_inliers > K || !cands[b].dpt_map_dev || !cands[b].kp_dpts0_dev || !cands[b].kp_homo0_dev ||
          !vcands[b].feat1_dev || !vcands[b].grad1_dev || !vcands[b].mask1_dev)
        return SAGE_E_INVALID;
      surv[ns++] = b;
    }
  }
  for (int b = 0; b < B; ++b)
    std::memset(&results[b], 0, sizeof(results[b]));
  if (ns == 0)
    return SAGE_OK;

  // 1. the survivors' keypoint terms: one launch
  const SageCamera &cam = query->pyr.cam[0];
  VerifyGatherParams G{};
  G.divisor0 = query_depth_divisor; G.cx = cam.cx; G.cy = cam.cy; G.fx = cam.fx; G.fy = cam.fy; G.Wf = (float)(int)cam.w;
  G.HW = (long long)cam.w * (long long)cam.h;
  G.K = K;
  int max_n = 0;
  for (int s = 0; s < ns; ++s)
  {
    const int b = surv[s];
    VerifyGatherItem &it = G.item[s];
    it.kp_homo0 = cands[b].kp_homo0_dev; it.kp_dpts0 = cands[b].kp_dpts0_dev; it.dpt_map = cands[b].dpt_map_dev;
    it.raw = raw_matched_loc1d + (size_t)b * K; it.inlier_kp = inlier_kp_dev + (size_t)b * K;
    it.out = kp_gathered_dev + (size_t)b * 8 * K; it.n = pre[b].reg.n_inliers;
    max_n = std::max(max_n, it.n);
  }
  hipLaunchKernelGGL(verify_gather_kernel, dim3((max_n + kBlock - 1) / kBlock, ns), dim3(kBlock), 0, ws->stream, G);
  SAGE_HIP(hipGetLastError());

  // 2.-4. start values, weights, one batch over the survivors (the gather is ahead of its launches in the stream)
  SageLmConfig lm = *cfg;
  lm.no_overlap_error = 0.f; // use_match_geom: the no-overlap exit is off (camera_tracker.cpp:1515)
  SageTrackProblem probs[SAGE_TRACK_MAX_BATCH];
  float pose12[SAGE_TRACK_MAX_BATCH * 12], scale[SAGE_TRACK_MAX_BATCH], err[SAGE_TRACK_MAX_BATCH];
  int iters[SAGE_TRACK_MAX_BATCH], status[SAGE_TRACK_MAX_BATCH];
  for (int s = 0; s < ns; ++s)
  {
    const int b = surv[s];
    const SageRegistrationResult &reg = pre[b].reg;
    const float *g = kp_gathered_dev + (size_t)b * 8 * K;
    SageTrackProblem &p = probs[s];
    std::memset(&p, 0, sizeof(p));
    p.ws = ws;
    p.use_photo = 1;
    p.mask1_dev = vcands[b].mask1_dev; p.dpts0_dev = query->unscaled_dpts0_dev; p.homo_dev = query->homo_dev;
    p.feat0s_dev = query->feat0s_dev; p.feat1_dev = vcands[b].feat1_dev; p.grad1_dev = vcands[b].grad1_dev;
    p.weights_dev = query->weights_dev; p.pyr = query->pyr; p.eps = query->eps; p.N = query->N; p.FS = query->FS;
    p.use_keypoints = 1; p.NK = reg.n_inliers;
    p.kp_homo0_dev = g; p.kp_dpts0_dev = g + 3 * (size_t)K; p.kp_matched_homo1_dev = g + 4 * (size_t)K;
    p.kp_matched_dpts1_dev = g + 7 * (size_t)K;
    p.kp_loss_param = vcands[b].kp_loss_param;
    p.kp_weight = pre[b].desc_match_inlier_ratio * match_geom_factor_weight; // :414, :742
    for (int i = 0; i < 9; ++i)
      pose12[12 * s + i] = (float)reg.R[i];
    for (int i = 0; i < 3; ++i)
      pose12[12 * s + 9 + i] = (float)reg.t[i];
    scale[s] = (float)reg.scale; // :750-761
  }
  int rc;
  if ((rc = sage_track_frame_batch(&lm, 7, probs, ns, pose12, scale, err, iters, status, nullptr, 0, nullptr)))
    return rc;

  // 5. overlap statistics of every tracked survivor: one batch, a row per survivor whose tracker returned SAGE_OK
  SageOverlapPose ov_pose[SAGE_TRACK_MAX_BATCH];
  SageOverlapStats ov[SAGE_TRACK_MAX_BATCH];
  int ov_of[SAGE_TRACK_MAX_BATCH], n_ov = 0;
  for (int s = 0; s < ns; ++s)
  {
    SageLoopVerifyResult &r = results[surv[s]];
    r.tracked = 1;
    r.status = status[s];
    std::memcpy(r.pose12, pose12 + 12 * s, sizeof(r.pose12));
    r.scale = scale[s];
    r.error = err[s];
    r.iters = iters[s];
    if (status[s] != SAGE_OK)
      continue;
    SageOverlapPose &q = ov_pose[n_ov];
    std::memcpy(q.R, r.pose12, sizeof(q.R));
    std::memcpy(q.t, r.pose12 + 9, sizeof(q.t));
    q.depth_scale = scale[s] / query_depth_divisor; // :1644
    ov_of[n_ov++] = surv[s];
  }
  if ((rc = sage_track_overlap_batch(ws, ov_pose, n_ov, query->valid_dpts0_dev, query->valid_homo_dev, query->M, &cam,
                                     query->mask_dev, query->eps, ov)))
    return rc;
  for (int i = 0; i < n_ov; ++i)
  {
    SageLoopVerifyResult &r = results[ov_of[i]];
    r.area_ratio = ov[i].area_ratio;
    r.inlier_ratio = ov[i].inlier_ratio;
    r.average_motion = ov[i].average_motion;
    r.area_inlier_ratio = ov[i].area_ratio * ov[i].inlier_ratio;
  }
  return SAGE_OK;
}

// the loop body behind the tracking stage and what follows the loop (loop_detector.cpp:173-229); the rules themselves are
// host functions of loop_accept_host.cpp
extern "C" int sage_loop_accept(SageWorkspace *ws, const SageLoopAcceptConfig *cfg, const SageLoopScaleQuery *query,
                                const SageLoopCandidate *cands, const SageLoopScaleCandidate *scands,
                                const SageLoopPrecheckResult *pre, const SageLoopVerifyResult *ver, int B, SageLoopInfo *infos,
                                int32_t *kept_order, int32_t *n_kept)
{
  if (!ws || !cfg || !query || !infos || !kept_order || !n_kept || B < 0 || B > SAGE_TRACK_MAX_BATCH)
    return SAGE_E_INVALID;
  if (B > 0 && (!cands || !scands || !pre || !ver))
    return SAGE_E_INVALID;
  int acc[SAGE_TRACK_MAX_BATCH], na = 0;
  for (int b = 0; b < B; ++b)
  {
    if (!loop_accept_test(*cfg, pre[b], ver[b]))
      continue;
    const SageLoopScaleCandidate &c = scands[b];
    if (!cands[b].dpt_map_dev || !c.valid_loc1d_dev || !c.valid_homo_dev || c.M <= 0 || !(c.dpt_scale > 0.f) ||
        !std::isfinite(c.dpt_scale) || !(c.tracker_ref_scale > 0.f) || !std::isfinite(c.tracker_ref_scale))
      return SAGE_E_INVALID;
    acc[na++] = b;
  }
  const SageCamera &cam = query->cam;
  if (na > 0 && (!query->bias_dev || !query->video_mask_dev || !depth_scale_camera_ok(&cam)))
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
  {
    std::memset(&infos[b], 0, sizeof(infos[b]));
    kept_order[b] = -1;
  }
  *n_kept = 0;
  if (na == 0)
    return SAGE_OK;

  // the accepted candidates' poses, then their depth-scale corrections: one batch, a row per accepted candidate
  SageDepthScaleRow rows[SAGE_TRACK_MAX_BATCH];
  SageDepthScaleStats stats[SAGE_TRACK_MAX_BATCH];
  for (int a = 0; a < na; ++a)
  {
    const int b = acc[a];
    SageLoopInfo &li = infos[b];
    li.accepted = 1;
    li.id_ref = scands[b].id;
    loop_accept_pose(ver[b].pose12, scands[b].dpt_scale, scands[b].tracker_ref_scale, li.R_cur_ref, li.t_cur_ref);
    li.ref_scale = scands[b].dpt_scale;
    li.desc_inlier_ratio = pre[b].desc_match_inlier_ratio;
    li.metric = ver[b].area_inlier_ratio;
    SageDepthScaleRow &r = rows[a];
    std::memset(&r, 0, sizeof(r));
    std::memcpy(r.R10, li.R_cur_ref, sizeof(r.R10));
    std::memcpy(r.t10, li.t_cur_ref, sizeof(r.t10));
    r.dpt0_dev = cands[b].dpt_map_dev; r.loc1d0_dev = scands[b].valid_loc1d_dev; r.homo0_dev = scands[b].valid_homo_dev;
    r.M = scands[b].M;
  }
  int rc;
  if ((rc = sage_depth_scale_ratio_batch(ws, rows, na, &cam, query->bias_dev, query->video_mask_dev, cfg->dpt_eps, 1, stats)))
    return rc;
  for (int a = 0; a < na; ++a)
  {
    infos[acc[a]].query_scale = stats[a].ratio;
    infos[acc[a]].scale = stats[a];
  }
  *n_kept = loop_accept_filter(infos, B, cfg->redundant_range, kept_order);
  return SAGE_OK;
}
