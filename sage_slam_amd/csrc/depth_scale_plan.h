// depth_scale_plan.h -- (no HIP) what the exact selection of depth_scale.hip keeps per row and the layout of a batch of rows
// (sage_depth_scale_ratio_batch, sage_median_f32_batch).  depth_scale_host.cpp holds the one definition of the layout; the
// public plan function and the batched calls in depth_scale.hip read it.
#pragma once

#include <cmath>
#include <cstdint>

#include "sage_ba.h"

constexpr int kSelBins = 2048;     // bins of the widest digit
constexpr int kSelPasses = 3;      // digits of 11 + 11 + 10 bits, from the top
constexpr int kSelMaxBlocks = 256; // workgroups of a row in the per-point and the histogram passes; the rest is grid-strided
constexpr int kSelBlock = 256;     // lanes of a workgroup (= kBlock)

struct SelState // what a pass hands to the next one
{
  uint32_t prefix; // the key's bits above the next digit
  uint32_t rank;   // the wanted rank among the keys under that prefix
};

struct SelHost // a row's pinned record
{
  float value;
  int32_t n_pos, n_selected, n_nan, n_used;
  int32_t pad[3];
};

// a row's device scratch: zero between calls (select_finish_kernel leaves it so)
struct SelScratch
{
  uint32_t hist[kSelPasses][kSelBins];
  int32_t cnt[4]; // |pos|, |selected|, NaNs among the selected
  SelState state[2];
};

constexpr int kSelFixedLaunches = 5; // the per-point (or keys) kernel, two digit passes, the finish, the ticket

struct SelBatchPlan
{
  int B = 0;
  int n[SAGE_DEPTH_SCALE_MAX_BATCH];        // the rows' sizes
  int blk0[SAGE_DEPTH_SCALE_MAX_BATCH + 1]; // the workgroups before row b in the flat (row, workgroup) list; blk0[B..] = all
  int64_t key0[SAGE_DEPTH_SCALE_MAX_BATCH]; // the row's first key in the keys allocation
  int64_t keys = 0;                         // the sum of the sizes
  int64_t device_bytes = 0, pinned_bytes = 0;
  int launches = 0, workgroups = 0;
};

inline int sel_blocks(int n) // the workgroups of a row of n
{
  const long long nb = ((long long)n + kSelBlock - 1) / kSelBlock;
  return nb < kSelMaxBlocks ? (int)nb : kSelMaxBlocks;
}
// n [B]: every entry > 0, 0 <= B <= SAGE_DEPTH_SCALE_MAX_BATCH (the caller has checked)
void sel_batch_plan(const int32_t *n, int B, SelBatchPlan *plan);

// the camera test of sage_depth_scale_ratio, its batch and sage_loop_accept: the one definition
inline bool depth_scale_camera_ok(const SageCamera *cam)
{
  return std::isfinite(cam->fx) && std::isfinite(cam->fy) && cam->fx > 0.f && cam->fy > 0.f && std::isfinite(cam->w) &&
         std::isfinite(cam->h) && cam->w >= 1.f && cam->h >= 1.f && !(cam->w > 32768.f) && !(cam->h > 32768.f);
}
