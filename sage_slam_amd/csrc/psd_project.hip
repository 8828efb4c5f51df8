// psd_project.hip -- batched Higham projection on the device: sage_nearest_psd (host_math.cpp, psd_mode 1) for n per-edge
// systems at once, one workgroup per matrix, everything in LDS and in fp64.
//
//   load     B = (M + M^T) / 2 widened from the fp32 row; a non-finite entry: B is written out as it is, status 2
//   eigen    B = V diag(w) V^T by parallel cyclic two-sided Jacobi: the D / 2 disjoint pairs of a round (psd_round_pair,
//            psd_project.h) are rotated at once, each by its own group of kPsdLanesPerPair lanes -- columns p, q of the work
//            matrix and rows p, q of V^T, a barrier, rows p, q of the work matrix, a barrier.  A sweep is psd_rounds(D)
//            rounds; before every sweep the off-diagonal and the diagonal sums of squares are measured, the sweeps end at
//            off <= (2^-52)^2 diag or at kPsdSweepCap (status 1)
//   project  H = V |w| V^T, A3 = (B + H) / 2 on the upper triangle, mirrored
//   accept   unpivoted right-looking LDL^T with the rule of is_psd (a negative pivot fails, a zero pivot zeroes its column --
//            here a column that is not zero already fails as well);
//            while it fails, at most kPsdBumpCap times, the diagonal is bumped as sage_nearest_psd bumps it.  The smallest
//            eigenvalue of A3 the bump starts from is min_k (w_k + |w_k|) / 2, the spectrum of A3 up to rounding
//            (status 3 when the last bump still was not accepted)
//   write    C [D][D] and the matrix's SagePsdStats
//
// No atomics, nothing outside the matrix's own rows is read or written, every loop has a fixed bound and every branch
// around a barrier is taken by the whole workgroup (it depends on values all lanes read from the same LDS words).
#include "runtime_internal.h"
#include "psd_project.h"

namespace
{

// sums of a and b over the workgroup, in a fixed order: down the lanes of a wave, then over the waves' slots in turn
__device__ inline void psd_block_sum2(double &a, double &b, double *slots, int tid, int nt)
{
  for (int o = 32; o > 0; o >>= 1)
  {
    a += __shfl_down(a, o);
    b += __shfl_down(b, o);
  }
  __syncthreads(); // (the slots' readers of the previous sum are through)
  if ((tid & 63) == 0)
  {
    slots[2 * (tid >> 6)] = a;
    slots[2 * (tid >> 6) + 1] = b;
  }
  __syncthreads();
  double sa = 0.0, sb = 0.0;
  for (int k = 0; k < (nt >> 6); ++k)
  {
    sa += slots[2 * k];
    sb += slots[2 * k + 1];
  }
  a = sa;
  b = sb;
}

// a matrix's record, the padding word after the three counters included: records compare byte for byte
static_assert(sizeof(SagePsdStats) == 32 && offsetof(SagePsdStats, min_eig) == 16, "device-visible layout");
__device__ inline void psd_write_stats(SagePsdStats *st, int status, int sweeps, int bumps, double min_eig, double off_norm)
{
  int32_t *head = reinterpret_cast<int32_t *>(st);
  head[0] = status;
  head[1] = sweeps;
  head[2] = bumps;
  head[3] = 0;
  st->min_eig = min_eig;
  st->off_norm = off_norm;
}

template <int DC>
__global__ __launch_bounds__(psd_threads(DC)) void psd_project_kernel(const float *__restrict__ AtA, double *__restrict__ C,
                                                                      SagePsdStats *__restrict__ stats, int D)
{
  constexpr int L = kPsdLanesPerPair, NT = psd_threads(DC), NG = NT / L;
  __shared__ double lds[psd_lds_doubles(DC)];
  __shared__ int s_bad;
  const int tid = threadIdx.x, g = tid / L, l = tid % L;
  const int S = psd_stride(D);
  const float *M = AtA + (size_t)blockIdx.x * D * D;
  double *Cout = C + (size_t)blockIdx.x * D * D;
  double *A = lds, *V = A + DC * (DC | 1), *w = V + DC * (DC | 1), *absw = w + DC, *col = absw + DC, *slots = w + 4 * DC;

  // ---- load: B into A, the identity into V (rows of V = eigenvectors: V^T)
  if (tid == 0)
    s_bad = 0;
  __syncthreads();
  bool bad = false;
  for (int i = g; i < D; i += NG)
    for (int j = l; j < D; j += L)
    {
      const double b = 0.5 * ((double)M[i * D + j] + (double)M[j * D + i]);
      A[i * S + j] = b;
      V[i * S + j] = i == j ? 1.0 : 0.0;
      bad = bad || !(fabs(b) <= 1.7976931348623157e308);
    }
  if (bad)
    s_bad = 1; // (every writer stores the same value)
  __syncthreads();
  if (s_bad)
  {
    for (int i = g; i < D; i += NG)
      for (int j = l; j < D; j += L)
        Cout[i * D + j] = A[i * S + j];
    if (tid == 0)
    {
      psd_write_stats(stats + blockIdx.x, 2, 0, 0, 0.0, 0.0);
    }
    return;
  }

  // ---- eigen-decomposition
  const int rounds = psd_rounds(D), np = D / 2;
  const double eps2 = 4.930380657631324e-32; // (2^-52)^2
  int sweeps = 0, status = 0;
  double off_exit = 0.0;
  for (int sweep = 0; sweep <= kPsdSweepCap; ++sweep)
  {
    double off = 0.0, dg = 0.0;
    for (int i = g; i < D; i += NG)
      for (int j = l; j < D; j += L)
      {
        const double v = A[i * S + j];
        if (i == j)
          dg += v * v;
        else
          off += v * v;
      }
    psd_block_sum2(off, dg, slots, tid, NT);
    off_exit = off;
    if (off <= eps2 * dg)
      break;
    if (sweep == kPsdSweepCap)
    {
      status = 1;
      break;
    }
    for (int r = 0; r < rounds; ++r)
    {
      // the group's rotation: every lane of the group computes it from the same three words (the rotation formula of
      // sym_eig).  The group lies inside one wave, so these reads come before any lane's writes below
      int p = 0, q = 0;
      double c = 1.0, s = 0.0, app_new = 0.0, aqq_new = 0.0;
      bool act = false;
      if (g < np)
      {
        psd_round_pair(D, r, g, &p, &q);
        const double apq = A[p * S + q];
        if (fabs(apq) >= 1e-300)
        {
          const double app = A[p * S + p], aqq = A[q * S + q];
          const double tau = (aqq - app) / (2.0 * apq);
          const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + t * t);
          s = t * c;
          // the rotated 2 x 2 block in closed form: its off-diagonal entry is zero, not the rounding residue of the two
          // products (a residue of eps |a_pp| per pair would keep `off` above the threshold for good)
          app_new = app - t * apq;
          aqq_new = aqq + t * apq;
          act = true;
        }
      }
      if (act)
        for (int k = l; k < D; k += L)
        {
          const double akp = A[k * S + p], akq = A[k * S + q];
          A[k * S + p] = c * akp - s * akq;
          A[k * S + q] = s * akp + c * akq;
          const double vp = V[p * S + k], vq = V[q * S + k];
          V[p * S + k] = c * vp - s * vq;
          V[q * S + k] = s * vp + c * vq;
        }
      __syncthreads();
      if (act)
        for (int k = l; k < D; k += L)
        {
          const double apk = A[p * S + k], aqk = A[q * S + k];
          A[p * S + k] = k == p ? app_new : (k == q ? 0.0 : c * apk - s * aqk);
          A[q * S + k] = k == q ? aqq_new : (k == p ? 0.0 : s * apk + c * aqk);
        }
      __syncthreads();
    }
    ++sweeps;
  }
  if (tid < D)
  {
    const double wk = A[tid * S + tid];
    w[tid] = wk;
    absw[tid] = fabs(wk);
  }
  __syncthreads();
  double min_eig = w[0], mn = 0.5 * (w[0] + absw[0]);
  for (int k = 1; k < D; ++k)
  {
    min_eig = fmin(min_eig, w[k]);
    mn = fmin(mn, 0.5 * (w[k] + absw[k]));
  }

  // ---- projection: A3 = (B + V |w| V^T) / 2 into A (the work matrix has been read for the last time)
  for (int i = g; i < D; i += NG)
    for (int j = i + l; j < D; j += L)
    {
      double h = 0.0;
      for (int k = 0; k < D; ++k)
        h += (V[k * S + i] * absw[k]) * V[k * S + j];
      const double b = 0.5 * ((double)M[i * D + j] + (double)M[j * D + i]);
      const double v = 0.5 * (b + h);
      A[i * S + j] = v;
      A[j * S + i] = v;
    }

  // ---- acceptance test and bump loop (sage_nearest_psd); V now holds the copy the LDL^T works on
  int bumps = 0;
  double kk = 1.0;
  bool accepted = false;
  for (int it = 0; it < kPsdBumpCap; ++it)
  {
    __syncthreads();
    for (int i = g; i < D; i += NG)
      for (int j = l; j <= i; j += L)
        V[i * S + j] = A[i * S + j];
    __syncthreads();
    bool ok = true;
    for (int j = 0; j < D; ++j)
    {
      const double d = V[j * S + j];
      if (d < 0.0)
      {
        ok = false;
        break;
      }
      if (d == 0.0)
      {
        // a zero pivot zeroes its column -- and the column has to be zero already: [[0, x], [x, 0]] is indefinite for any
        // x, and rounding residue of that shape is what a negative definite B leaves behind.  Stricter than is_psd, which
        // drops the column unseen
        if (tid == 0)
          s_bad = 0;
        __syncthreads();
        for (int i = j + 1 + tid; i < D; i += NT)
          if (V[i * S + j] != 0.0)
            s_bad = 1;
        __syncthreads();
        const bool nonzero = s_bad != 0;
        __syncthreads();
        if (nonzero)
        {
          ok = false;
          break;
        }
        continue;
      }
      for (int i = j + 1 + tid; i < D; i += NT)
        col[i] = V[i * S + j] / d;
      __syncthreads();
      for (int i = j + 1 + g; i < D; i += NG)
      {
        const double li = col[i];
        for (int k = j + 1 + l; k <= i; k += L)
          V[i * S + k] -= li * V[k * S + j];
      }
      __syncthreads();
    }
    if (ok)
    {
      accepted = true;
      break;
    }
    double dmax = 0.0;
    for (int i = 0; i < D; ++i)
      dmax = fmax(dmax, fabs(A[i * S + i]));
    const double ulp = dmax * 2.220446049250313e-16;
    double bump = -mn * kk + 1e-15;
    if (bump < ulp) // (the re-measured minimum of the host loop is the tracked one here: mn follows every bump exactly)
      bump = ulp;
    __syncthreads();
    if (tid < D)
      A[tid * S + tid] += bump;
    mn += bump;
    kk *= 2.0;
    ++bumps;
  }
  __syncthreads();
  if (!accepted && status == 0)
    status = 3; // (the host loop ends the same way, silently; here the window call hands such a factor to the host)

  // ---- write
  for (int i = g; i < D; i += NG)
    for (int j = l; j < D; j += L)
      Cout[i * D + j] = A[i * S + j];
  if (tid == 0)
  {
    psd_write_stats(stats + blockIdx.x, status, sweeps, bumps, min_eig, sqrt(off_exit));
  }
}

template <int DC>
void psd_launch(hipStream_t s, int D, int n, const float *AtA, double *C, SagePsdStats *stats)
{
  static_assert(sizeof(double) * psd_lds_doubles(DC) <= 163840, "a workgroup's LDS");
  hipLaunchKernelGGL((psd_project_kernel<DC>), dim3(n), dim3(psd_threads(DC)), 0, s, AtA, C, stats, D);
}

} // namespace

// n > 0 matrices of 1 <= D <= SAGE_PSD_MAX_DIM columns, one launch on `s`; stats: device-visible (device or pinned) [n]
int psd_project_enqueue(hipStream_t s, int D, int n, const float *AtA_dev, double *C_dev, SagePsdStats *stats)
{
  switch (psd_capacity(D))
  {
  case 16: psd_launch<16>(s, D, n, AtA_dev, C_dev, stats); break;
  case 32: psd_launch<32>(s, D, n, AtA_dev, C_dev, stats); break;
  case 48: psd_launch<48>(s, D, n, AtA_dev, C_dev, stats); break;
  case 64: psd_launch<64>(s, D, n, AtA_dev, C_dev, stats); break;
  case 80: psd_launch<80>(s, D, n, AtA_dev, C_dev, stats); break;
  default: return SAGE_E_INVALID;
  }
  SAGE_HIP(hipGetLastError());
  return SAGE_OK;
}

extern "C" int sage_factor_psd_batch(SageWorkspace *ws, int D, int n, const float *AtA_dev, double *C_dev,
                                     SagePsdStats *stats_host)
{
  int rc;
  if ((rc = psd_check_args(ws, D, n, AtA_dev, C_dev)))
    return rc;
  ws->psd_launches = 0;
  if (n == 0)
    return SAGE_OK;
  PsdPlan plan;
  psd_plan(D, n, &plan);
  if ((rc = ws->psd_host.reserve((size_t)plan.pinned_bytes)))
    return rc;
  SagePsdStats *rec = ws->psd_host.as<SagePsdStats>();
  if ((rc = psd_project_enqueue(ws->stream, D, n, AtA_dev, C_dev, rec)))
    return rc;
  if ((rc = ws_ticket_wait(ws)))
    return rc;
  ws->psd_launches = plan.launches;
  if (stats_host)
    std::memcpy(stats_host, rec, (size_t)plan.pinned_bytes);
  return SAGE_OK;
}

extern "C" int sage_factor_psd_batch_launches(const SageWorkspace *ws) { return ws ? ws->psd_launches : 0; }
