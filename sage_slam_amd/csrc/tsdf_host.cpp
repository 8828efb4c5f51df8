// tsdf_host.cpp -- (no HIP) the planning of a TSDF volume and the argument checks of its calls: the view frustum folded into
// running bounds, the voxel size that fits a voxel budget, the volume's dimensions (include/sage_ba.h "TSDF fusion").
#include "tsdf.h"

#include <cmath>

namespace sage
{
namespace tsdf
{

static bool camera_ok(const SageCamera &c)
{
  return std::isfinite(c.fx) && std::isfinite(c.fy) && std::isfinite(c.cx) && std::isfinite(c.cy) && c.fx > 0.f && c.fy > 0.f &&
         c.w >= 1.f && c.h >= 1.f && (double)(long long)c.w * (double)(long long)c.h < 2147483648.0;
}

int check_view(const SageTsdfView *v)
{
  if (!v || !v->depth_dev || !camera_ok(v->cam))
    return SAGE_E_INVALID;
  if (v->image_floats < (int64_t)v->cam.w * (int64_t)v->cam.h)
    return SAGE_E_INVALID;
  for (int i = 0; i < SAGE_POSE_FLOATS; ++i)
    if (!std::isfinite(v->pose12[i]))
      return SAGE_E_INVALID;
  if (!std::isfinite(v->obs_weight) || !(v->obs_weight > 0.f) || !std::isfinite(v->min_depth) || !std::isfinite(v->std_floor) ||
      v->std_floor < 0.f)
    return SAGE_E_INVALID;
  return SAGE_OK;
}

int check_batch(const SageTsdfView *views, int n, int flags)
{
  if (!views || n < 1 || n > kMaxViews || (flags & ~(SAGE_TSDF_NO_CULL | SAGE_TSDF_BRICK_X4)))
    return SAGE_E_INVALID;
  for (int i = 0; i < n; ++i)
    if (const int rc = check_view(views + i))
      return rc;
  return SAGE_OK;
}

} // namespace tsdf
} // namespace sage

using namespace sage::tsdf;

extern "C" int sage_tsdf_frustum_bounds(const SageCamera *cam, const float *pose12, double max_depth, double bounds[6])
{
  if (!cam || !pose12 || !bounds || !camera_ok(*cam) || !std::isfinite(max_depth))
    return SAGE_E_INVALID;
  for (int i = 0; i < SAGE_POSE_FLOATS; ++i)
    if (!std::isfinite(pose12[i]))
      return SAGE_E_INVALID;
  const double w = cam->w, h = cam->h;
  const double px[5] = {0, 0, 0, w, w}, py[5] = {0, 0, h, 0, h}, pd[5] = {0, max_depth, max_depth, max_depth, max_depth};
  for (int i = 0; i < 5; ++i)
  {
    const double c[3] = {(px[i] - (double)cam->cx) * pd[i] / (double)cam->fx, (py[i] - (double)cam->cy) * pd[i] / (double)cam->fy, pd[i]};
    for (int a = 0; a < 3; ++a)
    {
      const double x = ((double)pose12[3 * a + 0] * c[0] + (double)pose12[3 * a + 1] * c[1] + (double)pose12[3 * a + 2] * c[2]) +
                       (double)pose12[9 + a];
      bounds[a] = std::fmin(bounds[a], x);
      bounds[3 + a] = std::fmax(bounds[3 + a], x);
    }
  }
  return SAGE_OK;
}

extern "C" int sage_tsdf_plan(const double bounds[6], double base_voxel, double max_voxels, double trunc_multiplier, int with_color,
                              SageTsdfPlan *out)
{
  if (!bounds || !out || !std::isfinite(base_voxel) || !(base_voxel > 0.0) || !std::isfinite(trunc_multiplier) ||
      !(trunc_multiplier > 0.0) || std::isnan(max_voxels))
    return SAGE_E_INVALID;
  double ext[3];
  for (int a = 0; a < 3; ++a)
  {
    if (!std::isfinite(bounds[a]) || !std::isfinite(bounds[3 + a]) || !(bounds[3 + a] > bounds[a]))
      return SAGE_E_INVALID;
    ext[a] = bounds[3 + a] - bounds[a];
  }
  double voxel = base_voxel;
  if (max_voxels > 0.0)
  {
    const double volume = (ext[0] / base_voxel) * (ext[1] / base_voxel) * (ext[2] / base_voxel);
    voxel = base_voxel * std::cbrt(volume / max_voxels);
  }
  if (!std::isfinite(voxel) || !(voxel > 0.0))
    return SAGE_E_INVALID;
  double count = 1.0;
  SageTsdfPlan p{};
  for (int a = 0; a < 3; ++a)
  {
    const double d = std::ceil(ext[a] / voxel);
    if (!(d >= 1.0) || d > 2147483647.0)
      return SAGE_E_INVALID;
    p.dim[a] = (int32_t)d;
    p.origin[a] = (float)bounds[a];
    count *= d;
  }
  if (count > 2147483647.0)
    return SAGE_E_INVALID;
  p.with_color = with_color ? 1 : 0;
  p.voxel_size = (float)voxel;
  p.trunc_margin = (float)(voxel * trunc_multiplier);
  p.voxels = (int64_t)p.dim[0] * p.dim[1] * p.dim[2];
  p.device_bytes = p.voxels * (int64_t)sizeof(float) * (p.with_color ? 3 : 2) + bricks_of(p.dim, 1) * (int64_t)sizeof(int32_t);
  *out = p;
  return SAGE_OK;
}

extern "C" int sage_tsdf_integrate_batch_launches(int n) { return n >= 1 && n <= kMaxViews ? 1 : 0; }
extern "C" int sage_tsdf_view_chunk(void) { return kViewChunk; }
