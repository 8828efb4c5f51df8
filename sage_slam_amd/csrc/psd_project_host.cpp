// psd_project_host.cpp -- (no HIP) the host half of the batched Higham projection: the plan of a batch
// (sage_factor_psd_batch_plan), the argument checks sage_factor_psd_batch answers with before it touches the device, and the
// public face of the Jacobi schedule the kernel walks (sage_jacobi_round_pairs).  Nothing here touches the device.
#include "psd_project.h"

void psd_plan(int D, int n, PsdPlan *plan)
{
  PsdPlan &p = *plan;
  p = PsdPlan();
  p.D = D;
  p.n = n;
  p.capacity = psd_capacity(D);
  p.threads = psd_threads(p.capacity);
  p.lds_bytes = (int64_t)sizeof(double) * psd_lds_doubles(p.capacity);
  p.device_bytes = (int64_t)n * D * D * (int64_t)(sizeof(float) + sizeof(double));
  p.pinned_bytes = (int64_t)n * (int64_t)sizeof(SagePsdStats);
  p.launches = n > 0 ? 2 : 0; // the projection kernel, the ticket
}

int psd_check_args(const void *ws, int D, int n, const void *AtA_dev, const void *C_dev)
{
  if (!ws || !AtA_dev || !C_dev || D < 1 || D > SAGE_PSD_MAX_DIM || n < 0)
    return SAGE_E_INVALID;
  return SAGE_OK;
}

extern "C" int sage_factor_psd_batch_plan(int D, int n, int64_t *lds_bytes, int64_t *device_bytes, int64_t *pinned_bytes,
                                          int32_t *launches)
{
  if (D < 1 || D > SAGE_PSD_MAX_DIM || n < 0)
    return SAGE_E_INVALID;
  PsdPlan p;
  psd_plan(D, n, &p);
  if (lds_bytes)
    *lds_bytes = p.lds_bytes;
  if (device_bytes)
    *device_bytes = p.device_bytes;
  if (pinned_bytes)
    *pinned_bytes = p.pinned_bytes;
  if (launches)
    *launches = p.launches;
  return SAGE_OK;
}

extern "C" int sage_jacobi_round_pairs(int D, int round, int32_t *pairs)
{
  if (D < 1 || D > SAGE_PSD_MAX_DIM || round < 0 || round >= psd_rounds(D) || !pairs)
    return SAGE_E_INVALID;
  const int np = D / 2;
  for (int s = 0; s < np; ++s)
  {
    int p, q;
    psd_round_pair(D, round, s, &p, &q);
    pairs[2 * s] = p;
    pairs[2 * s + 1] = q;
  }
  return np;
}
