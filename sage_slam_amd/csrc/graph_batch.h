// graph_batch.h -- what the host units see of a window's pose-graph terms (graph_kernels.hip): the parameters and the launch
// of the batched kernel.  The arithmetic and the table row are graph_terms.h.
#pragma once

#include <hip/hip_runtime.h>

#include "graph_terms.h"
#include "term_results.h"

namespace sage
{

// lanes that share a term (14 of them own a row of AtA and an entry of Atb), terms per wave and per workgroup
constexpr int kGraphLanes = 16, kGraphBlock = 256;
constexpr int kGraphTermsPerWave = 64 / kGraphLanes, kGraphTermsPerBlock = kGraphBlock / kGraphLanes;

struct GraphBatchParams
{
  const GraphTerm *terms; // [n]
  int n;
  const float *vars; // [K][VS]: pose 12, scale, code CS -- the variable set being evaluated
  int VS;
  TermResults out;   // AtA / Atb (linearize only) of every kind's group by GraphTerm::out, {error, residuals} by GraphTerm::stat
};

// every local graph term of a window in ONE launch; jac = false: errors only
hipError_t launch_graph_terms(hipStream_t s, bool jac, const GraphBatchParams &p);

} // namespace sage
