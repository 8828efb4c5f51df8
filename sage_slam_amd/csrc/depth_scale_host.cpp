// depth_scale_host.cpp -- (no HIP) the layout of a batch of selections (sage_depth_scale_ratio_batch, sage_median_f32_batch;
// the public sage_depth_scale_ratio_batch_plan).  Nothing here touches the device.
#include "depth_scale_plan.h"

void sel_batch_plan(const int32_t *n, int B, SelBatchPlan *plan)
{
  SelBatchPlan &p = *plan;
  p = SelBatchPlan();
  p.B = B;
  int blocks = 0;
  int64_t keys = 0;
  for (int b = 0; b < SAGE_DEPTH_SCALE_MAX_BATCH; ++b)
  {
    p.n[b] = b < B ? n[b] : 0;
    p.blk0[b] = blocks;
    p.key0[b] = keys;
    if (b < B)
    {
      blocks += sel_blocks(n[b]);
      keys += n[b];
    }
  }
  p.blk0[SAGE_DEPTH_SCALE_MAX_BATCH] = blocks;
  p.keys = keys;
  p.workgroups = blocks;
  p.device_bytes = (int64_t)sizeof(uint32_t) * keys + (int64_t)sizeof(SelScratch) * B;
  p.pinned_bytes = (int64_t)sizeof(SelHost) * B;
  p.launches = B > 0 ? kSelFixedLaunches : 0;
}

extern "C" int sage_depth_scale_ratio_batch_plan(const int32_t *M, int B, int64_t *device_bytes, int64_t *pinned_bytes,
                                                 int32_t *launches, int32_t *workgroups)
{
  if (B < 0 || B > SAGE_DEPTH_SCALE_MAX_BATCH || (B > 0 && !M))
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
    if (M[b] <= 0)
      return SAGE_E_INVALID;
  SelBatchPlan p;
  sel_batch_plan(M, B, &p);
  if (device_bytes)
    *device_bytes = p.device_bytes;
  if (pinned_bytes)
    *pinned_bytes = p.pinned_bytes;
  if (launches)
    *launches = p.launches;
  if (workgroups)
    *workgroups = p.workgroups;
  return SAGE_OK;
}
