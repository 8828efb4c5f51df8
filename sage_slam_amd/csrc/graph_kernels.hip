// graph_kernels.hip -- the pose-graph terms of a window on the device: relative-pose-scale, relative-pose and scale-prior
// terms (graph_terms.h has the arithmetic), every local term of a window in one launch per linearize and one per error pass.
//
// A term is ~3 kflop and a K = 512 graph has ~3 000 of them, so a workgroup per term would be mostly idle: 16 lanes share a
// term, four terms a wave, sixteen a workgroup.  The lanes of a term evaluate its J [7][14] and residuals redundantly (the same
// instructions on the same inputs: the same bits), then lane i < 14 forms row i of AtA = w J^T J and entry i of Atb: 7-term
// sums in a fixed order, no atomics, no LDS, one writer per output -- bit-reproducible.  Every element of a term's [14][14],
// [14] and {error, residuals} is written by every launch (zeros included), so nothing needs clearing.
// J is held in registers and only ever indexed with compile-time constants (graph_normal_row picks a lane's column with a
// chain of selects), so the kernel has no scratch.
#include "graph_batch.h"

namespace sage
{

template <bool JAC>
__global__ __launch_bounds__(kGraphBlock) void graph_terms_kernel(const GraphBatchParams p)
{
  const int g = (int)(blockIdx.x * kGraphBlock + threadIdx.x) / kGraphLanes, lane = (int)threadIdx.x % kGraphLanes;
  if (g >= p.n)
    return;
  const GraphTerm t = p.terms[g];
  const float *x0 = p.vars + (size_t)t.k0 * p.VS, *x1 = p.vars + (size_t)t.k1 * p.VS;
  float pose0[12], pose1[12];
#pragma unroll
  for (int i = 0; i < 12; ++i)
  {
    pose0[i] = x0[i];
    pose1[i] = x1[i];
  }
  float J[kGraphRows][kGraphD], r[kGraphRows];
  const float err = graph_term_eval<JAC>(pose0, pose1, x0[12], x1[12], t, J, r);
  if (JAC && lane < kGraphD)
  {
    float row[kGraphD], b;
    graph_normal_row(J, r, t.weight, lane, row, b);
    constexpr int G = plan::graph_kind_group(0); // (every kind's)
    static_assert(TermResults::dim(G, 0) == kGraphD, "the graph terms' group");
    float *A = p.out.AtA(G) + (size_t)t.out * (kGraphD * kGraphD) + lane * kGraphD;
#pragma unroll
    for (int j = 0; j < kGraphD; ++j)
      A[j] = row[j];
    p.out.Atb(G)[(size_t)t.out * kGraphD + lane] = b;
  }
  if (lane == kGraphLanes - 1)
  {
    p.out.stats[2 * (size_t)t.stat + 0] = err;
    p.out.stats[2 * (size_t)t.stat + 1] = (float)graph_kind_rows(t.kind);
  }
}

hipError_t launch_graph_terms(hipStream_t s, bool jac, const GraphBatchParams &p)
{
  if (p.n <= 0)
    return hipSuccess;
  const int blocks = (p.n + kGraphTermsPerBlock - 1) / kGraphTermsPerBlock;
  if (jac)
    hipLaunchKernelGGL(graph_terms_kernel<true>, dim3(blocks), dim3(kGraphBlock), 0, s, p);
  else
    hipLaunchKernelGGL(graph_terms_kernel<false>, dim3(blocks), dim3(kGraphBlock), 0, s, p);
  return hipGetLastError();
}

} // namespace sage
