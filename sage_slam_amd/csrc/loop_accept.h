// loop_accept.h -- (no HIP) the host rules of sage_loop_accept (registration.hip): the accept test of loop_detector.cpp:165-183,
// the pose hand-over of camera_tracker.cpp:1651-1656 and loop_detector.cpp:189-193, the sort and the redundancy filter of
// :207-228.  include/sage_ba.h states the rules; loop_accept_host.cpp holds the one definition of each.
#pragma once

#include <cstdint>

#include "sage_ba.h"

// is candidate b accepted?  (a NaN fails every comparison)
bool loop_accept_test(const SageLoopAcceptConfig &cfg, const SageLoopPrecheckResult &pre, const SageLoopVerifyResult &ver);
// R_cur_ref = R^T, t_cur_ref = ((-R^T t) * dpt_scale) / tracker_ref_scale of the tracked pose12, fp32 without contraction
void loop_accept_pose(const float *pose12, float dpt_scale, float tracker_ref_scale, float *R_cur_ref, float *t_cur_ref);
// the accepted candidates by descending desc_inlier_ratio (ties keep candidate order), then the redundancy filter: sets
// infos[b].kept, writes the kept ones' indices in that order; returns their number
int loop_accept_filter(SageLoopInfo *infos, int B, int64_t redundant_range, int32_t *kept_order);
