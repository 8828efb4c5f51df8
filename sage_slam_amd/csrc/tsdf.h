// tsdf.h -- TSDF fusion (include/sage_ba.h "TSDF fusion"): what the host-only planning (tsdf_host.cpp) and the device side
// (tsdf.hip, window_tsdf.hip) share.  No HIP in here: tsdf_host.cpp is callable without a device.
#pragma once

#include <cstddef>
#include <cstdint>

#include "sage_ba.h"

namespace sage
{
namespace tsdf
{

constexpr int kMaxViews = 1024;   // views of one sage_tsdf_integrate_batch
constexpr int kViewChunk = 32;    // views staged in LDS at a time (sage_tsdf_view_chunk)
constexpr int kBrickZ = 64;       // a brick's long side: one wave, one line of 64 voxels along z
constexpr int kBrickY = 4;        // lines of a brick along y: the waves of its workgroup
constexpr int kBrickShapes = 3;   // bricks of 1, 2 or 4 voxels along x (voxels per thread): SAGE_TSDF_BRICK_X*
constexpr int kDefaultShape = 2;  // 4 x 4 x 64: DESIGN.md s3 "TSDF fusion" says why

// a brick's extent along x for the shape bits of `flags`, or 0 for bits that name no shape
inline int brick_x_of(int flags)
{
  const int sel = (flags >> 4) & 3;
  return sel == 0 ? (1 << kDefaultShape) : sel == 1 ? 1 : sel == 2 ? 2 : 4;
}
inline long long bricks_of(const int32_t dim[3], int brick_x)
{
  return (long long)((dim[0] + brick_x - 1) / brick_x) * ((dim[1] + kBrickY - 1) / kBrickY) * ((dim[2] + kBrickZ - 1) / kBrickZ);
}

// SAGE_OK or SAGE_E_INVALID for one view: NULL depth, a camera without positive fx / fy / w / h (or w * h >= 2^31), images of
// fewer floats than w * h, a pose, intrinsic or scalar that is not finite, obs_weight <= 0, std_floor < 0
int check_view(const SageTsdfView *v);
// ... for the arguments of a batch, the views included
int check_batch(const SageTsdfView *views, int n, int flags);

} // namespace tsdf
} // namespace sage
