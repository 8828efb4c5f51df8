// relin_host.cpp -- (no HIP) the stateless halves of the partial relinearization behind the C ABI: the reads table applied to
// two variable sets (sage_relin_plan) and gtsam's relinearization check (sage_relin_marks).  The rules are relin_plan.h's.
#include "relin_plan.h"
#include "sage_ba.h"

using namespace sage;

extern "C" int sage_relin_plan(int K, int CS, int n_links, const int32_t *links, const float *pose_old, const float *code_old,
                               const float *scale_old, const float *pose_new, const float *code_new, const float *scale_new,
                               uint8_t *photo_stale, uint8_t *geo_stale, uint8_t *map_read, int32_t *n_photo, int32_t *n_geo)
{
  if (K < 1 || CS < 1 || n_links < 0 || (n_links > 0 && !links) || !pose_old || !code_old || !scale_old || !pose_new ||
      !code_new || !scale_new || !photo_stale || !geo_stale || !map_read)
    return SAGE_E_INVALID;
  for (int l = 0; l < n_links; ++l)
    if (links[2 * l] < 0 || links[2 * l] >= K || links[2 * l + 1] < 0 || links[2 * l + 1] >= K || links[2 * l] == links[2 * l + 1])
      return SAGE_E_INVALID;
  const std::vector<uint8_t> ch = plan::changed_groups(K, CS, pose_old, code_old, scale_old, pose_new, code_new, scale_new);
  std::memset(map_read, 0, (size_t)K);
  int32_t np = 0, ng = 0;
  for (int e = 0; e < 2 * n_links; ++e)
  {
    int src, dst;
    plan::edge_ends(links, e, &src, &dst);
    photo_stale[e] = plan::photo_edge_stale(ch[src], ch[dst]);
    geo_stale[e] = plan::geo_edge_stale(ch[src], ch[dst]);
    plan::edge_map_reads(src, dst, photo_stale[e], geo_stale[e], map_read, nullptr);
    np += photo_stale[e];
    ng += geo_stale[e];
  }
  if (n_photo)
    *n_photo = np;
  if (n_geo)
    *n_geo = ng;
  return SAGE_OK;
}

extern "C" int sage_relin_marks(const double *delta, int K, int CS, const SageRelinThresholds *t, int32_t *marks,
                                int32_t *n_marked)
{
  if (!delta || !t || !marks || K < 1 || CS < 1)
    return SAGE_E_INVALID;
  int32_t n = 0;
  for (int k = 0; k < K; ++k)
  {
    const uint8_t m = plan::relin_marks_of(delta + (size_t)k * (7 + CS), CS, t->pose, t->code, t->scale);
    marks[k] = m;
    n += (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1);
  }
  if (n_marked)
    *n_marked = n;
  return SAGE_OK;
}
