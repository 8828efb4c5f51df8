// depth_sigma.hip -- per-pixel depth uncertainty of a batch of keyframes: with d(p) = s (bias(p) + basis(p,:) code), its
// Jacobian j = [s basis(p,:) (CS), bias(p) + basis(p,:) code] against (code, scale) and S their marginal covariance,
//   var(p) = j^T S j,   sigma(p) = sqrtf(max(var, 0)).
// The kernel reads the bytes depth_batch_kernel (producers.hip) reads -- 4 (CS + 2) per pixel with its output -- and spends
// ~(CS + 1)(CS + 2) / 2 multiply-adds per pixel on them; HBM is the bound ("Marginal covariances").
// No atomics, one writer per output, a fixed summation order: bit-reproducible.
#include "runtime_internal.h"
#include "sage_device.h"

namespace sage
{

struct DepthSigmaDev // a row of the launch's table
{
  const float *bias, *basis, *code, *scale_dev, *S; // S: fp32 [(CS + 1)][(CS + 1)], symmetric
  float *out;
  float scale;
  int pad;
};

constexpr int kSigmaPixels = 256; // per workgroup: one pixel per thread

// grid (pixel tiles, keyframes).  The tile's basis rows arrive as coalesced 16-byte pieces (consecutive threads, consecutive
// addresses; all of a thread's loads in flight together) and are laid into LDS in rows of CS + 4 floats, S beside them, once
// per workgroup.  Thread p reads row p back with ds_read_b128, conflict-free: the 16-byte slots of 16 lanes whose ids differ
// mod 16 are 4 (9 p mod 16) for CS 32 and 4 (5 p mod 16) for CS 16, all different.  Every thread then walks the lower triangle
// of S (rows of CS + 4 floats, every lane the same address: broadcasts):
//   var = sum_i j_i (S_ii j_i + 2 sum_{k<i} S_ik j_k)
// at most 3 (CS + 1) + 2 roundings on any path.  A form that left the code-code part to v_mfma_f32_32x32x2_f32 (the tile's
// rows against S_cc, the row-wise dot through an LDS image of the products) was built and measured next to this one: 78.5 us
// against 55.9 us on the 64-keyframe 128 x 160 window (profiles/covariance_bench.txt) -- it cannot use the symmetry of S and
// pays for the column reads and the second LDS image; it was deleted.
template <int CS>
__global__ __launch_bounds__(kSigmaPixels) void depth_sigma_kernel(const DepthSigmaDev *__restrict__ items, int HW, int mode)
{
  constexpr int F4 = CS / 4, NS = CS + 1, SP = CS + 4, RS = CS + 4;
  __shared__ __attribute__((aligned(16))) float s_tile[kSigmaPixels * RS];
  __shared__ __attribute__((aligned(16))) float s_S[NS * SP];
  __shared__ float s_code[CS];
  const DepthSigmaDev it = items[blockIdx.y];
  const int tid = threadIdx.x, px0 = blockIdx.x * kSigmaPixels;
  f32x4 piece[F4];
#pragma unroll
  for (int u = 0; u < F4; ++u)
  {
    const int q = tid + kSigmaPixels * u, gp = px0 + q / F4;
    piece[u] = gp < HW ? *reinterpret_cast<const f32x4 *>(it.basis + (size_t)gp * CS + (q % F4) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int gp = px0 + tid;
  const float bias = gp < HW ? it.bias[gp] : 0.f;
  const float s = it.scale_dev ? it.scale_dev[0] : it.scale;
  for (int idx = tid; idx < NS * NS; idx += kSigmaPixels)
    s_S[(idx / NS) * SP + idx % NS] = it.S[idx];
  if (tid < CS)
    s_code[tid] = it.code[tid];
#pragma unroll
  for (int u = 0; u < F4; ++u)
  {
    const int q = tid + kSigmaPixels * u;
    float *dst = s_tile + (q / F4) * RS + (q % F4) * 4;
    *reinterpret_cast<f32x4 *>(dst) = piece[u];
  }
  __syncthreads();
  float j[NS];
#pragma unroll
  for (int q = 0; q < F4; ++q)
  {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(s_tile + tid * RS + 4 * q);
    j[4 * q + 0] = v[0]; j[4 * q + 1] = v[1]; j[4 * q + 2] = v[2]; j[4 * q + 3] = v[3];
  }
  float d0 = bias;
#pragma unroll
  for (int i = 0; i < CS; ++i)
  {
    d0 = fmaf(j[i], s_code[i], d0);
    j[i] *= s;
  }
  j[CS] = d0;
  float var = 0.f;
#pragma unroll
  for (int i = 0; i < NS; ++i)
  {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < i; ++k)
      acc = fmaf(s_S[i * SP + k], j[k], acc);
    var = fmaf(j[i], fmaf(2.f, acc, s_S[i * SP + i] * j[i]), var);
  }
  if (gp < HW)
    it.out[gp] = mode == SAGE_DEPTH_SIGMA ? sqrtf(fmaxf(var, 0.f)) : var;
}

} // namespace sage

int depth_sigma_enqueue(hipStream_t s, DepthSigmaStage &stage, const DepthSigmaEntry *e, int n, int H, int W, int CS, int mode,
                        hipEvent_t before, hipEvent_t after)
{
  const int HW = H * W, NS = CS + 1;
  const size_t table_bytes = ((size_t)n * sizeof(DepthSigmaDev) + 15) / 16 * 16, bytes = table_bytes + (size_t)n * NS * NS * sizeof(float);
  int rc;
  if (stage.busy) // the last call's copy has left the pinned side?
    SAGE_HIP(hipEventSynchronize(stage.copied));
  stage.busy = false;
  if ((rc = stage.host.reserve(bytes)) || (rc = stage.dev.reserve(bytes)))
    return rc;
  if (!stage.copied)
    SAGE_HIP(hipEventCreateWithFlags(&stage.copied, hipEventDisableTiming));
  DepthSigmaDev *table = stage.host.as<DepthSigmaDev>();
  float *Sf = reinterpret_cast<float *>(stage.host.as<char>() + table_bytes);
  const float *Sdev = reinterpret_cast<const float *>(stage.dev.as<char>() + table_bytes);
  for (int i = 0; i < n; ++i)
  {
    table[i] = DepthSigmaDev{e[i].bias, e[i].basis, e[i].code, e[i].scale_dev, Sdev + (size_t)i * NS * NS, e[i].out, e[i].scale, 0};
    for (int r = 0; r < NS; ++r) // symmetrised in double, rounded once
      for (int c = 0; c < NS; ++c)
        Sf[((size_t)i * NS + r) * NS + c] = (float)(0.5 * (e[i].S[r * e[i].ldS + c] + e[i].S[c * e[i].ldS + r]));
  }
  SAGE_HIP(hipMemcpyAsync(stage.dev.p, stage.host.p, bytes, hipMemcpyHostToDevice, s));
  SAGE_HIP(hipEventRecord(stage.copied, s));
  stage.busy = true;
  const dim3 grid((HW + kSigmaPixels - 1) / kSigmaPixels, n);
  if (before)
    SAGE_HIP(hipEventRecord(before, s));
  if (CS == 32)
    hipLaunchKernelGGL((depth_sigma_kernel<32>), grid, dim3(kSigmaPixels), 0, s, stage.dev.as<DepthSigmaDev>(), HW, mode);
  else
    hipLaunchKernelGGL((depth_sigma_kernel<16>), grid, dim3(kSigmaPixels), 0, s, stage.dev.as<DepthSigmaDev>(), HW, mode);
  SAGE_HIP(hipGetLastError());
  if (after)
    SAGE_HIP(hipEventRecord(after, s));
  return SAGE_OK;
}

extern "C" int sage_depth_sigma_batch(SageWorkspace *ws, const SageDepthSigmaItem *items, int n, int H, int W, int CS, int mode)
{
  if (!ws || !items || n < 1 || H < 1 || W < 1 || (mode != SAGE_DEPTH_VARIANCE && mode != SAGE_DEPTH_SIGMA))
    return SAGE_E_INVALID;
  if (CS != 16 && CS != 32)
    return SAGE_E_UNSUPPORTED;
  if (n > 65535)
    return SAGE_E_INVALID;
  std::vector<DepthSigmaEntry> e(n);
  for (int i = 0; i < n; ++i)
  {
    const SageDepthSigmaItem &it = items[i];
    if (!it.bias_dev || !it.basis_dev || !it.code_dev || !it.cov_code_scale || !it.out_dev)
      return SAGE_E_INVALID;
    e[i] = DepthSigmaEntry{it.bias_dev, it.basis_dev, it.code_dev, nullptr, it.scale, it.cov_code_scale, (size_t)CS + 1, it.out_dev};
  }
  return depth_sigma_enqueue(ws->stream, ws->sigma, e.data(), n, H, W, CS, mode);
}
