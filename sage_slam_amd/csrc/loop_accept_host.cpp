// loop_accept_host.cpp -- (no HIP) the host rules of sage_loop_accept: the accept test of loop_detector.cpp:165-183, the pose
// hand-over of camera_tracker.cpp:1651-1656 and loop_detector.cpp:189-193, the sort and the redundancy filter of :207-228.
// include/sage_ba.h states the rules; nothing here touches the device.
#include "loop_accept.h"

#include <algorithm>

bool loop_accept_test(const SageLoopAcceptConfig &cfg, const SageLoopPrecheckResult &pre, const SageLoopVerifyResult &ver)
{
  if (!ver.tracked || ver.status != SAGE_OK) // :165
    return false;
  if (!(ver.area_ratio >= cfg.min_area_ratio) || !(ver.inlier_ratio >= cfg.min_inlier_ratio)) // :173
    return false;
  return ver.area_inlier_ratio >= cfg.base_metric && pre.desc_match_inlier_ratio >= cfg.base_desc_ratio; // :183
}

void loop_accept_pose(const float *pose12, float dpt_scale, float tracker_ref_scale, float *R_cur_ref, float *t_cur_ref)
{
#pragma STDC FP_CONTRACT OFF
  const float *R = pose12, *t = pose12 + 9;
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j)
      R_cur_ref[3 * i + j] = R[3 * j + i];
    const float a = (-R[0 + i]) * t[0], b = (-R[3 + i]) * t[1], c = (-R[6 + i]) * t[2];
    const float ti = (a + b) + c;
    const float scaled = ti * dpt_scale;
    t_cur_ref[i] = scaled / tracker_ref_scale;
  }
}

int loop_accept_filter(SageLoopInfo *infos, int B, int64_t redundant_range, int32_t *kept_order)
{
  int order[SAGE_TRACK_MAX_BATCH], n = 0;
  for (int b = 0; b < B; ++b)
  {
    kept_order[b] = -1;
    infos[b].kept = 0;
    if (infos[b].accepted)
      order[n++] = b;
  }
  std::stable_sort(order, order + n, [&](int l, int r) { return infos[l].desc_inlier_ratio > infos[r].desc_inlier_ratio; });
  int n_kept = 0;
  for (int i = 0; i < n; ++i)
  {
    bool add = true;
    for (int k = 0; k < n_kept && add; ++k)
    {
      const int64_t d = infos[kept_order[k]].id_ref - infos[order[i]].id_ref;
      add = !((d < 0 ? -d : d) < redundant_range);
    }
    if (add)
    {
      infos[order[i]].kept = 1;
      kept_order[n_kept++] = order[i];
    }
  }
  return n_kept;
}
