// relin_plan.h -- which of a window's dense edges a change of its variables makes stale, and ISAM2's relinearization check, as
// pure host arithmetic.  Standard library only -- no HIP: relin_host.cpp exports both through the C ABI, the window's stale-mode
// linearize (window_relin.hip) applies the same three steps to its snapshot, and tests/test_relin_host.py restates the table.
//
// Who reads what.  A directed edge a -> b (source a; global id 2 * link + direction, direction 0 = from the link's lower
// keyframe) reads
//   photometric   pose a, pose b, code a, scale a            the depth map of a
//   geometric     pose, code and scale of both               the depth maps of a and b, the gradient of b's
// "Changed" = the float bits differ (memcmp, the rule of sage_window_prepass): -0.0f against 0.0f is a change.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace sage
{
namespace plan
{

enum : uint8_t { kChangedPose = 1, kChangedCode = 2, kChangedScale = 4 }; // (the bits of SAGE_HOLD_*)

// step 1: per keyframe, the groups whose bits differ between two variable sets: pose [K][12], code [K][CS], scale [K]
inline std::vector<uint8_t> changed_groups(int K, int CS, const float *pose_old, const float *code_old, const float *scale_old,
                                           const float *pose_new, const float *code_new, const float *scale_new)
{
  std::vector<uint8_t> ch((size_t)K, 0);
  for (int k = 0; k < K; ++k)
  {
    if (std::memcmp(pose_old + (size_t)k * 12, pose_new + (size_t)k * 12, 12 * sizeof(float)) != 0)
      ch[k] |= kChangedPose;
    if (std::memcmp(code_old + (size_t)k * CS, code_new + (size_t)k * CS, (size_t)CS * sizeof(float)) != 0)
      ch[k] |= kChangedCode;
    if (std::memcmp(scale_old + k, scale_new + k, sizeof(float)) != 0)
      ch[k] |= kChangedScale;
  }
  return ch;
}

// step 2: the reads table.  Is the photometric / the geometric edge src -> dst stale, given the changed groups of its ends?
inline bool photo_edge_stale(uint8_t ch_src, uint8_t ch_dst) { return ch_src != 0 || (ch_dst & kChangedPose) != 0; }
inline bool geo_edge_stale(uint8_t ch_src, uint8_t ch_dst) { return ch_src != 0 || ch_dst != 0; }

// step 3: the depth maps the stale edges read.  map_read / grad_read [K] are OR-ed into (the caller zeroes them)
inline void edge_map_reads(int src, int dst, bool photo_stale, bool geo_stale, uint8_t *map_read, uint8_t *grad_read)
{
  if (photo_stale || geo_stale)
    map_read[src] = 1;
  if (geo_stale)
  {
    map_read[dst] = 1;
    if (grad_read)
      grad_read[dst] = 1;
  }
}

// the ends of directed edge 2 * link + dir of a link list [n_links][2] (either order of a link's keyframes)
inline void edge_ends(const int32_t *links, int edge, int *src, int *dst)
{
  const int a = links[2 * (edge / 2)], b = links[2 * (edge / 2) + 1];
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  *src = (edge & 1) ? hi : lo;
  *dst = (edge & 1) ? lo : hi;
}

// ---- gtsam's CheckRelinearizationFull with per-key vector thresholds (ISAM2-impl.h:345-372): a key is relinearized when
//      any |delta_i| > threshold_i, strictly -- a NaN compares false and marks nothing.  delta: one keyframe's B = 7 + CS rows
//      in block order (pose 6, code CS, scale); pose_thr [6]
inline uint8_t relin_marks_of(const double *delta, int CS, const float *pose_thr, float code_thr, float scale_thr)
{
  auto over = [](double d, float t) { return (d < 0 ? -d : d) > (double)t; };
  uint8_t m = 0;
  for (int i = 0; i < 6; ++i)
    if (over(delta[i], pose_thr[i]))
      m |= kChangedPose;
  for (int i = 0; i < CS; ++i)
    if (over(delta[6 + i], code_thr))
      m |= kChangedCode;
  if (over(delta[6 + CS], scale_thr))
    m |= kChangedScale;
  return m;
}

} // namespace plan
} // namespace sage
