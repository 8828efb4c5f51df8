// term_results.h -- where the terms of a window (keypoint and pose-graph terms) put their results, as the kernels that write
// them (keypoint_kernels.hip, graph_kernels.hip) and the ones that read them (window_eval.hip) see it: per group
// (window_plan.h) the AtA / Atb buffers, one {error, inliers} array, the entries per group.  TermSide (window_state.h) fills
// it; the indices into it are plan::term_layout's.
#pragma once

#include "damped_system.h" // SAGE_HD
#include "window_plan.h"

namespace sage
{

struct TermResults
{
  float *AtA0, *Atb0, *AtA1, *Atb1, *AtA2, *Atb2; // per group [count][D * D], [count][D]
  float *stats;                                   // [n_stats][2] of the pass; null: a window without terms
  int count0, count1, count2;
  // (select chains, not arrays: a dynamically indexed array of a by-value kernel argument may be spilled to scratch)
  SAGE_HD float *AtA(int group) const { return group == 0 ? AtA0 : (group == 1 ? AtA1 : AtA2); }
  SAGE_HD float *Atb(int group) const { return group == 0 ? Atb0 : (group == 1 ? Atb1 : Atb2); }
  SAGE_HD static constexpr int dim(int group, int CS) { return plan::term_group_dim(group, CS); }
  // the stat array's two runs: [0, n_photo_stats) rides in the photometric error total, the rest in the geometric one
  SAGE_HD int n_photo_stats() const { return count0; }
  SAGE_HD int n_geo_stats() const { return count1 + count2; }
};

// column map (= group) of an adjacency entry: a dense edge's type is its own, a term's is 2 + group
SAGE_HD constexpr int adj_group(int type) { return type == 4 ? 2 : (type & 1); }

} // namespace sage
