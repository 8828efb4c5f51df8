// match_batch.hip -- the loop detector's access pattern of the matching core: sage_cycle_match_batch, one query descriptor
// map against B candidate maps (LoopDetector::DetectLoop / DetectLocalLoop, core/system/loop_detector.cpp:143-163, :282-319,
// run CameraTracker::MatchGeoCheck on one query keyframe against up to 20 / 9 candidates one after the other).  Row b of every
// output is what sage_cycle_match writes for (query, candidate b, keypoints b), bit for bit: the response of a (query, pixel)
// pair is formed exactly as best_match_kernel (keypoint_kernels.hip) forms it -- channels ascending,
// __fadd_rn(acc, __fmul_rn(d, d)), no contraction -- and the winner is the maximum under ONE total order, larger response
// first, then smaller pixel index, which is what that kernel's per-lane '>' and its cross-lane tree compute together.
//
//   match_batch_kernel<0>  grid (pixel slice, query group, candidate): a workgroup holds kMbKPB query descriptors in LDS (read
//                          back 4 channels at a time), streams ITS contiguous pixel slice of the candidate's map, two pixels per
//                          lane and step, and writes per query the slice's first maximum as a (response, pixel) pair into
//                          part[pass 0][b][slice][k]
//   match_batch_kernel<1>  the way back: the same grid; the queries are candidate b's descriptors at the merged winners of
//                          pass 0 (every workgroup merges the slices' pairs of its own queries, 32 lanes per query; the
//                          workgroups of slice 0 also write raw_matched), the target is the one query map (1.3 MB: L2)
//   match_flags_kernel     a workgroup per candidate: merges pass 1's pairs (coalesced over k), writes cyc_matched and the
//                          flag, counts; the count goes into the workspace's pinned record and the workgroup that finishes last
//                          posts the ticket
// Three launches for any B and any number of slices, one wait, no copy.  The merge is a max under a total order of pairs whose
// pixel indices are all different, so its result does not depend on the order of the merge or on the split; no float atomics,
// one integer counter (who is last), plain C++ stores only.
#include "runtime_internal.h"

namespace
{
constexpr int kMbKPB = 8;            // queries per workgroup, as best_match_kernel: 8 accumulators x 2 pixels per lane
constexpr int kMbStep = 2 * kBlock;  // pixels a workgroup takes per step
constexpr int kMbMaxSlices = 8192;   // bound of a forced split (the pairs take 16 B K S bytes)
constexpr int kMbNoPixel = 0x7fffffff;

struct MbPair // a slice's (or the map's) first maximum of one query
{
  float r;
  int p;
};

struct MbArgs
{
  const float *cand[SAGE_MATCH_MAX_BATCH];   // candidate b's descriptor map
  const long long *kp[SAGE_MATCH_MAX_BATCH]; // candidate b's keypoints: pixels of the query map
  const float *query;
  MbPair *part;       // [2][B][S][K]
  long long *raw_out; // [B][K]
  int B, K, C, HW, S, slice_len;
};

__device__ __forceinline__ bool mb_better(float r2, int p2, float r, int p) { return r2 > r || (r2 == r && p2 < p); }

// the two pixels' squared distances to the workgroup's kMbKPB queries over the channels [c0, c0 + NC), added to acc in
// ascending channel order
template <int NC>
__device__ __forceinline__ void mb_accumulate(const float *__restrict__ s_q, int C, int c0, const float (&t0)[NC],
                                              const float (&t1)[NC], float (&acc0)[kMbKPB], float (&acc1)[kMbKPB])
{
#pragma unroll
  for (int kk = 0; kk < kMbKPB; ++kk)
  {
    float q[NC];
    if constexpr (NC == 4)
    {
      const float4 v = *reinterpret_cast<const float4 *>(s_q + kk * C + c0); // (C % 4 == 0 on this path: 16-byte aligned)
      q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
    }
    else
      q[0] = s_q[kk * C + c0];
#pragma unroll
    for (int j = 0; j < NC; ++j)
    {
      const float d0 = q[j] - t0[j], d1 = q[j] - t1[j];
      acc0[kk] = __fadd_rn(acc0[kk], __fmul_rn(d0, d0)); // no FMA contraction: the argmax must not depend on it
      acc1[kk] = __fadd_rn(acc1[kk], __fmul_rn(d1, d1));
    }
  }
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void match_batch_kernel(const MbArgs A)
{
  extern __shared__ __align__(16) float s_mb[]; // [kMbKPB][C] query descriptors, then the reduction scratch
  __shared__ long long s_loc[kMbKPB];
  float *s_q = s_mb;
  const int tid = threadIdx.x, K = A.K, C = A.C, HW = A.HW, S = A.S;
  const int slice = blockIdx.x, b = blockIdx.z, k0 = blockIdx.y * kMbKPB;
  const int nk = min(kMbKPB, K - k0);
  const float *__restrict__ qmap = PASS == 0 ? A.query : A.cand[b];
  const float *__restrict__ tmap = PASS == 0 ? A.cand[b] : A.query;

  // where the workgroup's queries sit in qmap
  if (PASS == 0)
  {
    if (tid < kMbKPB)
      s_loc[tid] = tid < nk ? A.kp[b][k0 + tid] : -1;
  }
  else
  {
    // the winner of pass 0 over all slices: 32 lanes per query over the slices, then the lanes
    const int kk = tid >> 5, l = tid & 31;
    float r = -INFINITY;
    int p = kMbNoPixel;
    if (kk < nk)
    {
      const MbPair *part = A.part + (size_t)b * S * K + (k0 + kk);
      for (int s = l; s < S; s += 32)
      {
        const MbPair m = part[(size_t)s * K];
        if (mb_better(m.r, m.p, r, p))
        {
          r = m.r;
          p = m.p;
        }
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
    {
      const float r2 = __shfl_xor(r, o, 64);
      const int p2 = __shfl_xor(p, o, 64);
      if (mb_better(r2, p2, r, p))
      {
        r = r2;
        p = p2;
      }
    }
    if (l == 0)
    {
      s_loc[kk] = kk < nk ? (long long)p : -1;
      if (kk < nk && slice == 0)
        A.raw_out[(size_t)b * K + k0 + kk] = p;
    }
  }
  __syncthreads();
  for (int i = tid; i < kMbKPB * C; i += kBlock)
  {
    const int kk = i / C, c = i - kk * C;
    const long long loc = s_loc[kk];
    s_q[i] = (loc >= 0 && loc < HW) ? qmap[(size_t)c * HW + loc] : 0.f; // (a location outside the map reads nothing)
  }
  __syncthreads();

  float best_r[kMbKPB];
  int best_p[kMbKPB];
#pragma unroll
  for (int kk = 0; kk < kMbKPB; ++kk)
  {
    best_r[kk] = -INFINITY;
    best_p[kk] = kMbNoPixel;
  }
  const int lo = slice * A.slice_len, hi = min(lo + A.slice_len, HW);
  for (int p0 = lo + tid; p0 < hi; p0 += kMbStep)
  {
    const int p1 = p0 + kBlock;
    const bool has1 = p1 < hi;
    const int q1 = has1 ? p1 : p0; // (the second pixel of a short step is the first again: computed, never compared)
    float acc0[kMbKPB], acc1[kMbKPB];
#pragma unroll
    for (int kk = 0; kk < kMbKPB; ++kk)
      acc0[kk] = acc1[kk] = 0.f;
    if ((C & 3) == 0)
      for (int c = 0; c < C; c += 4)
      {
        float t0[4], t1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
          t0[j] = tmap[(size_t)(c + j) * HW + p0];
          t1[j] = tmap[(size_t)(c + j) * HW + q1];
        }
        mb_accumulate<4>(s_q, C, c, t0, t1, acc0, acc1);
      }
    else
      for (int c = 0; c < C; ++c)
      {
        const float t0[1] = {tmap[(size_t)c * HW + p0]}, t1[1] = {tmap[(size_t)c * HW + q1]};
        mb_accumulate<1>(s_q, C, c, t0, t1, acc0, acc1);
      }
#pragma unroll
    for (int kk = 0; kk < kMbKPB; ++kk)
    {
      const float r0 = -acc0[kk], r1 = -acc1[kk];
      if (r0 > best_r[kk]) // ascending pixels per lane: '>' keeps the first maximum
      {
        best_r[kk] = r0;
        best_p[kk] = p0;
      }
      if (has1 && r1 > best_r[kk])
      {
        best_r[kk] = r1;
        best_p[kk] = p1;
      }
    }
  }

  // cross-lane: larger response wins, equal responses -> smaller index.  Within the wave by shuffles, then the four waves
  float *s_r = s_mb + kMbKPB * C;
  int *s_p = reinterpret_cast<int *>(s_r + kMbKPB * kWaves);
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int kk = 0; kk < kMbKPB; ++kk)
  {
    float r = best_r[kk];
    int p = best_p[kk];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
      const float r2 = __shfl_xor(r, o, 64);
      const int p2 = __shfl_xor(p, o, 64);
      if (mb_better(r2, p2, r, p))
      {
        r = r2;
        p = p2;
      }
    }
    if (lane == 0)
    {
      s_r[kk * kWaves + wave] = r;
      s_p[kk * kWaves + wave] = p;
    }
  }
  __syncthreads();
  if (tid < nk)
  {
    float r = s_r[tid * kWaves];
    int p = s_p[tid * kWaves];
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
    {
      const float r2 = s_r[tid * kWaves + w];
      const int p2 = s_p[tid * kWaves + w];
      if (mb_better(r2, p2, r, p))
      {
        r = r2;
        p = p2;
      }
    }
    MbPair m;
    m.r = r;
    m.p = p;
    A.part[(((size_t)PASS * A.B + b) * S + slice) * K + k0 + tid] = m;
  }
}

// per candidate: the winners of pass 1 over the slices, the flags (cycle_flags_kernel's expression) and their count
__global__ __launch_bounds__(kBlock) void match_flags_kernel(const MbArgs A, int W, float thresh, long long *__restrict__ cyc_out,
                                                             int32_t *__restrict__ flags, int32_t *host_counts, unsigned *done,
                                                             volatile unsigned *ticket, unsigned epoch)
{
  __shared__ int s_cnt[kWaves];
  const int tid = threadIdx.x, b = blockIdx.x, K = A.K, S = A.S;
  const MbPair *part = A.part + ((size_t)A.B + b) * S * K;
  const long long *__restrict__ kp = A.kp[b];
  int n = 0;
  for (int k = tid; k < K; k += kBlock)
  {
    float r = -INFINITY;
    int p = kMbNoPixel;
    for (int s = 0; s < S; ++s)
    {
      const MbPair m = part[(size_t)s * K + k];
      if (mb_better(m.r, m.p, r, p))
      {
        r = m.r;
        p = m.p;
      }
    }
    const long long loc0 = kp[k], cyc = p;
    const float dx = (float)(loc0 % W) - (float)(cyc % W);
    const float dy = (float)(loc0 / W) - (float)(cyc / W);
    const int in = (dx * dx + dy * dy) <= thresh * thresh; // match_geometry_factor.cpp:91-94
    cyc_out[(size_t)b * K + k] = cyc;
    flags[(size_t)b * K + k] = in;
    n += in;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    n += __shfl_down(n, o, 64);
  if ((tid & 63) == 0)
    s_cnt[tid >> 6] = n;
  __syncthreads();
  if (tid == 0)
  {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
      total += s_cnt[w];
    host_counts[b] = total;
    __threadfence_system(); // the count is on its way before this workgroup is counted as done
    if (atomicAdd(done, 1u) == (unsigned)A.B - 1u)
    {
      *done = 0; // (the next call's launch comes after this kernel)
      __threadfence_system();
      *ticket = epoch;
    }
  }
}
} // namespace

extern "C" int sage_cycle_match_batch(SageWorkspace *ws, const float *desc_query_dev, const float *const *desc_cand_dev,
                                      const int64_t *const *kp_loc1d_dev, int B, int K, int C, int H, int W, float cyc_thresh,
                                      int pixel_slices, int64_t *raw_matched_loc1d, int64_t *cyc_matched_loc1d,
                                      int32_t *inlier_flags, int32_t *n_inliers_host)
{
  if (!ws || B < 0 || B > SAGE_MATCH_MAX_BATCH || K < 0 || C < 1 || C > 1024 || H < 1 || W < 1 || pixel_slices < 0 ||
      (long long)H * W > 0x7fffffffll || (B > 0 && !n_inliers_host))
    return SAGE_E_INVALID;
  if (B > 0 && K > 0)
  {
    if (!desc_query_dev || !desc_cand_dev || !kp_loc1d_dev || !raw_matched_loc1d || !cyc_matched_loc1d || !inlier_flags)
      return SAGE_E_INVALID;
    for (int b = 0; b < B; ++b)
      if (!desc_cand_dev[b] || !kp_loc1d_dev[b])
        return SAGE_E_INVALID;
  }
  for (int b = 0; b < B; ++b)
    n_inliers_host[b] = 0;
  if (B == 0 || K == 0)
    return SAGE_OK;

  const int HW = H * W, groups = (K + kMbKPB - 1) / kMbKPB;
  if (groups > 65535)
    return SAGE_E_INVALID; // (the grid's second dimension: K <= 524 280)
  if (ws->mb_cus == 0)
  {
    int dev = 0, cus = 0;
    SAGE_HIP(hipGetDevice(&dev));
    SAGE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    ws->mb_cus = std::max(cus, 1);
  }
  // the split: as many slices as it takes to put two workgroups on every CU, none shorter than one step of a workgroup
  int S = pixel_slices;
  if (S == 0)
  {
    const int wgs = groups * B, want = 2 * ws->mb_cus;
    S = std::min((want + wgs - 1) / wgs, std::max(HW / kMbStep, 1));
  }
  S = std::min(S, std::min(HW, kMbMaxSlices));
  const int slice_len = (HW + S - 1) / S;
  S = (HW + slice_len - 1) / slice_len; // (no empty slice)
  ws->mb_slices = S;

  int rc;
  const size_t part_bytes = 2 * (size_t)B * S * K * sizeof(MbPair);
  if ((rc = ws->mb_part.reserve(part_bytes)) || (rc = ws->mb_host.reserve(SAGE_MATCH_MAX_BATCH * sizeof(int32_t))))
    return rc;
  hipStream_t s = ws->stream;
  if (!ws->mb_done.p)
  {
    if ((rc = ws->mb_done.reserve(sizeof(unsigned))))
      return rc;
    SAGE_HIP(hipMemsetAsync(ws->mb_done.p, 0, sizeof(unsigned), s)); // (from here on the flags kernel leaves it zero)
  }
  MbArgs A{};
  for (int b = 0; b < B; ++b)
  {
    A.cand[b] = desc_cand_dev[b];
    A.kp[b] = reinterpret_cast<const long long *>(kp_loc1d_dev[b]);
  }
  A.query = desc_query_dev;
  A.part = ws->mb_part.as<MbPair>();
  A.raw_out = reinterpret_cast<long long *>(raw_matched_loc1d);
  A.B = B; A.K = K; A.C = C; A.HW = HW; A.S = S; A.slice_len = slice_len;
  const size_t shm = ((size_t)kMbKPB * C + 2 * kMbKPB * kWaves) * sizeof(float);
  const dim3 grid(S, groups, B);
  hipLaunchKernelGGL(match_batch_kernel<0>, grid, dim3(kBlock), shm, s, A);
  hipLaunchKernelGGL(match_batch_kernel<1>, grid, dim3(kBlock), shm, s, A);
  const unsigned epoch = ws_ticket_next(ws);
  hipLaunchKernelGGL(match_flags_kernel, dim3(B), dim3(kBlock), 0, s, A, W, cyc_thresh, reinterpret_cast<long long *>(cyc_matched_loc1d),
                     inlier_flags, ws->mb_host.as<int32_t>(), ws->mb_done.as<unsigned>(), &ws->hs()->ticket, epoch);
  SAGE_HIP(hipGetLastError());
  if ((rc = ws_ticket_await(ws, epoch)))
    return rc;
  std::memcpy(n_inliers_host, ws->mb_host.p, (size_t)B * sizeof(int32_t));
  return SAGE_OK;
}

extern "C" int sage_cycle_match_batch_slices(const SageWorkspace *ws) { return ws ? ws->mb_slices : 0; }
