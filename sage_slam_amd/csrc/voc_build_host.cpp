// voc_build_host.cpp -- (no HIP) the host-only parts of sage_vocabulary_build: the counter-based draws, the argument checks,
// the plan, DBoW2's node numbering and the weights from the document counts.  include/sage_ba.h, "training the vocabulary",
// states every rule; voc_build.hip holds the device side and the level loop.
#include "voc_build.h"

#include <algorithm>
#include <cmath>

#include "sage_ba.h"

namespace sage_voc
{
int vb_check_shape(int C, long long M, int k, int L)
{
  if (k < 2 || L < 1 || C < 1 || M < 1)
    return SAGE_E_INVALID;
  if (C > kVbMaxC || k > kVbMaxK || L > kVbMaxL || M >= (1LL << 31))
    return SAGE_E_UNSUPPORTED;
  long long words = 1;
  for (int l = 0; l < L; ++l)
    if ((words *= k) > kVbMaxWords)
      return SAGE_E_UNSUPPORTED;
  return SAGE_OK;
}

int vb_plan(int C, long long M, int k, int L, VbPlan *p)
{
  const int rc = vb_check_shape(C, M, k, L);
  if (rc)
    return rc;
  long long kL1 = 1; // k^(L-1) <= 2^20 / 2
  for (int l = 1; l < L; ++l)
    kL1 *= k;
  p->Cp = 4 * ((C + 3) / 4);
  p->W = kL1 * k;
  p->A = std::min(kL1, std::max(1LL, M / 2));
  p->T = M / kVbTile + std::min(kL1, std::max(1LL, M / (k + 1)));
  const long long Cp = p->Cp, A = p->A, T = p->T;
  p->device_bytes = M * (4 * Cp + 8 + 4 + 4 + 4 + 4 + 4) + 8 * A * k * Cp + 4 * A + T * (8LL * k * C + 4 * k + 4 * k + 4 + 8) +
                    4 * p->W + 16 + kVbFlagBytes;
  p->pinned_bytes = 32 * A + 8 * T + 16 * A + 4 * A * k + 4 * A * k + 4 * A * k * Cp;
  return SAGE_OK;
}

void vb_number(const std::vector<VbRawNode> &raw, std::vector<int32_t> &id_of_raw, std::vector<int32_t> &order)
{
  id_of_raw.assign(raw.size(), -1);
  order.clear();
  order.reserve(raw.size());
  if (raw.empty())
    return;
  id_of_raw[0] = 0;
  order.push_back(0);
  // HKmeansStep: the children are created (consecutive ids), then each split child is finished in child order, depth-first:
  // an explicit stack of (node, next child to visit)
  std::vector<std::pair<int32_t, int32_t>> stack;
  auto finish = [&](int32_t r) {
    for (int32_t c = 0; c < raw[r].n_children; ++c)
    {
      id_of_raw[raw[r].first_child + c] = (int32_t)order.size();
      order.push_back(raw[r].first_child + c);
    }
    stack.emplace_back(r, 0);
  };
  finish(0);
  while (!stack.empty())
  {
    auto &top = stack.back();
    if (top.second >= raw[top.first].n_children)
    {
      stack.pop_back();
      continue;
    }
    const int32_t child = raw[top.first].first_child + top.second++;
    if (raw[child].n_children > 0)
      finish(child);
  }
}

void vb_weights(int weighting, int n_docs, const std::vector<int32_t> &ni, std::vector<double> &w)
{
  w.assign(ni.size(), 0.0);
  for (size_t i = 0; i < ni.size(); ++i)
    if (weighting == SAGE_VOC_TF || weighting == SAGE_VOC_BINARY)
      w[i] = 1.0;
    else if (ni[i] > 0)
      w[i] = std::log((double)n_docs / (double)ni[i]);
}
} // namespace sage_voc

using namespace sage_voc;

extern "C" void sage_vocabulary_build_config_default(SageVocabularyBuildConfig *cfg)
{
  if (!cfg)
    return;
  cfg->k = 10;
  cfg->L = 4;
  cfg->weighting = SAGE_VOC_TF_IDF;
  cfg->scoring = SAGE_BOW_L1;
  cfg->max_iterations = 100;
  cfg->seed = 0;
}

extern "C" uint64_t sage_vocabulary_build_draw(uint64_t seed, const int32_t *path, int depth, int j)
{
  return vb_draw(vb_path_hash(seed, path, path ? std::max(depth, 0) : 0), j);
}

extern "C" int sage_vocabulary_build_plan(int C, int64_t M, int k, int L, int64_t *device_bytes, int64_t *pinned_bytes,
                                          int32_t *launches_per_seed_round, int32_t *launches_per_lloyd_round)
{
  VbPlan p;
  const int rc = vb_plan(C, M, k, L, &p);
  if (rc)
    return rc;
  if (device_bytes)
    *device_bytes = p.device_bytes;
  if (pinned_bytes)
    *pinned_bytes = p.pinned_bytes;
  if (launches_per_seed_round)
    *launches_per_seed_round = 2;
  if (launches_per_lloyd_round)
    *launches_per_lloyd_round = 2;
  return SAGE_OK;
}
