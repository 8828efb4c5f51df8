// bow.hip -- the loop detector's bag of words: sage_vocabulary_* and sage_bow_transform.  LoopDetector::AddKeyframe
// (loop_detector.cpp:20-42) gathers the descriptors of a keyframe's valid pixels and hands them to
// TemplatedTensorVocabulary::transform (tensor_vocabulary.cpp:131-245), which walks the vocabulary tree recursively on the
// host: per inner node visited an index, a [C,S,k] broadcast subtraction, a sum and an argmin, per child a nonzero and a
// blocking .item().  Here it is a per-point descent with the gather fused in:
//
//   bow_walk_kernel      one lane per point: the descriptor is read once (desc[ch * P + loc[i]]) and kept in registers; at
//                        every node the nearest child by sum_ch (f - c)^2 (the difference form, the first smallest wins, a
//                        NaN counts as smallest), down to a leaf; the leaf's word is flagged with a plain store
//                        (hit[word] = 1: idempotent, no atomic).  The workgroup first stages as many whole breadth-first
//                        levels of the tree as fit kBowLdsBudget into LDS; deeper levels are read from global memory
//   bow_compact_kernel   one workgroup: scans hit[0, n_words), writes the words reached in ascending order and their number
//                        into the workspace's pinned record, clears the flags for the next call, posts the ticket
//   host finish          drops the leaves of weight <= 0, v = weight * M, L1-normalised by the sequential ascending sum
//                        (BowVector::normalize): the same operations in the same order as the reference, a function of the
//                        set of words reached alone
// Two launches, one ticket wait, no copy; what crosses PCIe is the words reached (4 bytes each).  No float atomics, no
// workgroup waits for another; every loop is bounded by the tree's depth, a node's fan-out, M or the number of words.
#include "runtime_internal.h"
#include "sage_device.h"

namespace
{
constexpr int kBowLdsBudget = 96 * 1024; // bytes of LDS a workgroup may fill with the tree's top levels (of 160 KiB per CU:
                                         // one workgroup per CU then, which is what a keyframe's M / 256 workgroups need)
constexpr int kBowMaxC = 64, kBowMaxFanout = 64, kBowMaxDepth = 8, kBowMaxWords = 1 << 20;
constexpr int kBowMaxBlocks = 2048;          // workgroups of the walk; the rest is grid-strided
constexpr int kBowScanTile = kBlock * 4;     // words per step of the compaction: hit[] is allocated in multiples of it

struct BowNode // breadth-first numbering: a node's children are contiguous
{
  int32_t child_begin, child_count; // child_count == 0: a leaf
  int32_t leaf_word;                // -1 for an inner node
};

struct BowHost // the pinned record
{
  int32_t n_hit;
  int32_t pad[3];
  int32_t ids[1]; // [n_words of the vocabulary]
};

struct BowWalkParams
{
  const float *desc;  // [C, P]
  const int64_t *loc; // [M] or null
  long long P;
  int M;
  const float4 *voc_desc; // [n_nodes][Cp4]
  const BowNode *nodes;   // [n_nodes]
  int C, Cp4, n_staged, depth;
  uint32_t *hit;      // [n_words]
  int32_t *word_out;  // [M] or null
};

// the nearest of the n children whose descriptor rows start at `rows`; f: the point's descriptor, zero beyond C like the rows
template <int CP4, bool EXACT>
__device__ __forceinline__ int bow_nearest(const float (&f)[CP4 * 4], const float4 *rows, int n, int cp4)
{
  int best = 0;
  float best_d = 0.0f;
#pragma unroll 2
  for (int j = 0; j < n; ++j)
  {
    const float4 *r = rows + (size_t)j * (EXACT ? CP4 : cp4);
    float d = 0.0f;
#pragma unroll
    for (int q = 0; q < CP4; ++q)
      if (EXACT || q < cp4)
      {
        const float4 v = r[q];
        const float e0 = f[4 * q + 0] - v.x, e1 = f[4 * q + 1] - v.y, e2 = f[4 * q + 2] - v.z, e3 = f[4 * q + 3] - v.w;
        d += e0 * e0;
        d += e1 * e1;
        d += e2 * e2;
        d += e3 * e3;
      }
    // torch.argmin: the first smallest; a NaN is smaller than everything, the first NaN stays
    if (j == 0 || d < best_d || (d != d && best_d == best_d))
    {
      best_d = d;
      best = j;
    }
  }
  return best;
}

// CP4: float4 groups of a descriptor held in registers; EXACT: the vocabulary's rows have exactly CP4 groups (C = 16, 32),
// otherwise any C <= 4 * CP4 (the generic path: the groups beyond the vocabulary's are skipped, uniformly)
template <int CP4, bool EXACT>
__global__ __launch_bounds__(kBlock) void bow_walk_kernel(const BowWalkParams P)
{
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  float4 *s_desc = reinterpret_cast<float4 *>(s_dyn);                                       // [n_staged][Cp4]
  int32_t *s_node = reinterpret_cast<int32_t *>(s_dyn + (size_t)P.n_staged * P.Cp4 * 4);    // [n_staged] BowNode
  const int tid = threadIdx.x;
  for (int i = tid; i < P.n_staged * P.Cp4; i += kBlock)
    s_desc[i] = P.voc_desc[i];
  {
    const int32_t *g = reinterpret_cast<const int32_t *>(P.nodes);
    for (int i = tid; i < P.n_staged * 3; i += kBlock)
      s_node[i] = g[i];
  }
  __syncthreads(); // (the only barrier: lanes without a point may leave below)
  const int cp4 = EXACT ? CP4 : P.Cp4;
  for (long long base = (long long)blockIdx.x * kBlock; base < P.M; base += (long long)gridDim.x * kBlock)
  {
    const long long i = base + tid;
    if (i >= P.M)
      break;
    const long long at = P.loc ? (long long)P.loc[i] : i; // (not range-checked: sage_ba.h)
    float f[CP4 * 4];
#pragma unroll
    for (int ch = 0; ch < CP4 * 4; ++ch)
      f[ch] = (EXACT || ch < P.C) ? P.desc[(long long)ch * P.P + at] : 0.0f;
    int node = 0, word = -1;
    for (int level = 0; level <= P.depth; ++level) // (a leaf is at most `depth` steps down)
    {
      BowNode nd;
      if (node < P.n_staged)
      {
        nd.child_begin = s_node[3 * node + 0];
        nd.child_count = s_node[3 * node + 1];
        nd.leaf_word = s_node[3 * node + 2];
      }
      else
        nd = P.nodes[node];
      if (nd.child_count == 0)
      {
        word = nd.leaf_word;
        break;
      }
      // whole levels are staged: a node's children are all in LDS or all in global memory
      const int best = nd.child_begin < P.n_staged
                           ? bow_nearest<CP4, EXACT>(f, s_desc + (size_t)nd.child_begin * cp4, nd.child_count, cp4)
                           : bow_nearest<CP4, EXACT>(f, P.voc_desc + (size_t)nd.child_begin * cp4, nd.child_count, cp4);
      node = nd.child_begin + best;
    }
    if (word >= 0) // (always: the tree was validated at creation)
      P.hit[word] = 1u;
    if (P.word_out)
      P.word_out[i] = word;
  }
}

__global__ __launch_bounds__(kBlock) void bow_compact_kernel(uint32_t *hit, int n_words, BowHost *host, volatile unsigned *ticket,
                                                             unsigned epoch)
{
  __shared__ int s_wave[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int total = 0; // the same in every thread
  for (int base = 0; base < n_words; base += kBowScanTile)
  {
    const int w0 = base + 4 * tid;
    uint4 *slot = reinterpret_cast<uint4 *>(hit + w0); // (hit[] is a multiple of the tile, zero beyond n_words)
    const uint4 h = *slot;
    const int cnt = (h.x != 0u) + (h.y != 0u) + (h.z != 0u) + (h.w != 0u);
    int inc = cnt; // inclusive sum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o)
        inc += t;
    }
    if (lane == 63)
      s_wave[wave] = inc;
    __syncthreads();
    int before = total, tile = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w)
    {
      if (w < wave)
        before += s_wave[w];
      tile += s_wave[w];
    }
    if (cnt)
    {
      int at = before + inc - cnt;
      if (h.x)
        host->ids[at++] = w0;
      if (h.y)
        host->ids[at++] = w0 + 1;
      if (h.z)
        host->ids[at++] = w0 + 2;
      if (h.w)
        host->ids[at++] = w0 + 3;
      *slot = make_uint4(0u, 0u, 0u, 0u); // the next call starts from zero
    }
    total += tile;
    __syncthreads(); // (s_wave is written again)
  }
  if (tid == 0)
    host->n_hit = total;
  __threadfence_system();
  __syncthreads();
  if (tid == 0)
  {
    __threadfence_system();
    *ticket = epoch;
  }
}

using BowWalkFn = void (*)(const BowWalkParams);
BowWalkFn bow_walk_for(int C)
{
  if (C == 16)
    return bow_walk_kernel<4, true>;
  if (C == 32)
    return bow_walk_kernel<8, true>;
  return bow_walk_kernel<kBowMaxC / 4, false>;
}
} // namespace

struct SageVocabulary
{
  int n_nodes = 0, n_words = 0, C = 0, Cp4 = 0, depth = 0, max_fanout = 0;
  int n_staged = 0;       // nodes (whole breadth-first levels from the root) the walk stages in LDS
  size_t lds_bytes = 0;   // ... and what they take
  // host side of the finish: per word its weight and its leaf, per node (breadth-first) its parent
  std::vector<double> word_weight;
  std::vector<int32_t> word_leaf, parent_bfs;
  DevBuf nodes, desc; // BowNode [n_nodes], float [n_nodes][4 * Cp4]
};

extern "C" int sage_vocabulary_create(const SageVocabularyDesc *d, SageVocabulary **out)
{
  if (!d || !out || !d->parent || !d->descriptors || !d->weight || !d->word_id || d->n_nodes < 2 || d->C < 1 ||
      d->scoring < SAGE_BOW_L1 || d->scoring > SAGE_BOW_DOT_PRODUCT)
    return SAGE_E_INVALID;
  const int n = d->n_nodes;
  if (d->parent[0] != -1)
    return SAGE_E_INVALID;
  std::vector<int32_t> n_children(n, 0), level(n, 0);
  int depth = 0;
  for (int i = 1; i < n; ++i)
  {
    const int32_t p = d->parent[i];
    if (p < 0 || p >= i)
      return SAGE_E_INVALID;
    ++n_children[p];
    level[i] = level[p] + 1;
    depth = std::max(depth, (int)level[i]);
  }
  int n_words = 0, max_fanout = 0;
  for (int i = 0; i < n; ++i)
  {
    max_fanout = std::max(max_fanout, (int)n_children[i]);
    if (n_children[i] == 0)
      ++n_words;
    if ((n_children[i] == 0) != (d->word_id[i] >= 0) || d->word_id[i] < -1) // a word id exactly on the leaves; -1 elsewhere
      return SAGE_E_INVALID;
  }
  if (n_words < 1)
    return SAGE_E_INVALID;
  std::vector<int32_t> word_node(n_words, -1);
  for (int i = 0; i < n; ++i)
    if (n_children[i] == 0)
    {
      const int32_t w = d->word_id[i];
      if (w >= n_words || word_node[w] >= 0) // outside 0..n_words-1, or twice: no permutation
        return SAGE_E_INVALID;
      word_node[w] = i;
    }
  if (d->C > kBowMaxC || max_fanout > kBowMaxFanout || depth > kBowMaxDepth || n_words > kBowMaxWords || d->scoring != SAGE_BOW_L1)
    return SAGE_E_UNSUPPORTED;

  // breadth-first numbering; children by ascending node index (i runs upwards)
  std::vector<int32_t> child_first(n + 1, 0), children(n > 1 ? n - 1 : 0);
  for (int i = 0; i < n; ++i)
    child_first[i + 1] = child_first[i] + n_children[i];
  {
    std::vector<int32_t> fill(child_first.begin(), child_first.end() - 1);
    for (int i = 1; i < n; ++i)
      children[fill[d->parent[i]]++] = i;
  }
  std::vector<int32_t> order, bfs_of(n, -1); // order[b]: the node at breadth-first position b
  order.reserve(n);
  order.push_back(0);
  for (size_t b = 0; b < order.size(); ++b)
    for (int32_t c = child_first[order[b]]; c < child_first[order[b] + 1]; ++c)
      order.push_back(children[c]);
  if ((int)order.size() != n) // (cannot happen: every node has a path to the root through smaller indices)
    return SAGE_E_INVALID;
  for (int b = 0; b < n; ++b)
    bfs_of[order[b]] = b;

  SageVocabulary *v = new SageVocabulary();
  v->n_nodes = n; v->n_words = n_words; v->C = d->C; v->Cp4 = (d->C + 3) / 4; v->depth = depth; v->max_fanout = max_fanout;
  const int Cp = 4 * v->Cp4;
  std::vector<BowNode> nodes(n);
  std::vector<float> desc((size_t)n * Cp, 0.0f);
  v->word_weight.resize(n_words);
  v->word_leaf.resize(n_words);
  v->parent_bfs.assign(n, -1);
  for (int b = 0; b < n; ++b)
  {
    const int i = order[b];
    nodes[b].child_count = n_children[i];
    nodes[b].child_begin = n_children[i] ? bfs_of[children[child_first[i]]] : 0;
    nodes[b].leaf_word = n_children[i] ? -1 : d->word_id[i];
    if (i > 0)
    {
      v->parent_bfs[b] = bfs_of[d->parent[i]];
      std::memcpy(&desc[(size_t)b * Cp], d->descriptors + (size_t)i * d->C, (size_t)d->C * sizeof(float));
    }
    if (!n_children[i])
    {
      v->word_weight[d->word_id[i]] = d->weight[i];
      v->word_leaf[d->word_id[i]] = b;
    }
  }
  auto fail = [&](int rc) {
    delete v;
    return rc;
  };
  int ndev = 0, lds_max = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1)
    return fail(e != hipSuccess ? (int)e : (int)hipErrorNoDevice);
  int device = 0;
  if ((e = hipGetDevice(&device)) != hipSuccess ||
      (e = hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device)) != hipSuccess)
    return fail((int)e);
  // the levels staged in LDS: the longest prefix of whole levels within the budget (breadth-first: a level is a run)
  long long budget = std::min(kBowLdsBudget, lds_max);
  if (const char *env = std::getenv("SAGE_BOW_LDS_BUDGET")) // measurement: scripts/bow_bench.py runs the walk without staging
    budget = std::max(0LL, std::min(budget, std::atoll(env)));
  const size_t per_node = (size_t)Cp * sizeof(float) + sizeof(BowNode);
  {
    int end = 0; // nodes of the levels 0..l
    for (int l = 0; l <= depth; ++l)
    {
      while (end < n && level[order[end]] == l)
        ++end;
      if ((long long)((size_t)end * per_node) <= budget)
        v->n_staged = end;
      else
        break;
    }
  }
  v->lds_bytes = (size_t)v->n_staged * per_node;
  int rc;
  if ((rc = v->nodes.reserve(nodes.size() * sizeof(BowNode))) || (rc = v->desc.reserve(desc.size() * sizeof(float))))
    return fail(rc);
  if ((e = hipMemcpy(v->nodes.p, nodes.data(), nodes.size() * sizeof(BowNode), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(v->desc.p, desc.data(), desc.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
    return fail((int)e);
  if (v->lds_bytes > 48 * 1024) // more dynamic LDS than a kernel gets without asking
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void *>(bow_walk_for(v->C)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)v->lds_bytes)) != hipSuccess)
      return fail((int)e);
  *out = v;
  return SAGE_OK;
}

extern "C" void sage_vocabulary_destroy(SageVocabulary *voc) { delete voc; }
extern "C" int sage_vocabulary_num_nodes(const SageVocabulary *voc) { return voc ? voc->n_nodes : -1; }
extern "C" int sage_vocabulary_num_words(const SageVocabulary *voc) { return voc ? voc->n_words : -1; }
extern "C" int sage_vocabulary_channels(const SageVocabulary *voc) { return voc ? voc->C : -1; }
extern "C" int sage_vocabulary_depth(const SageVocabulary *voc) { return voc ? voc->depth : -1; }
extern "C" int sage_vocabulary_max_fanout(const SageVocabulary *voc) { return voc ? voc->max_fanout : -1; }
extern "C" int sage_vocabulary_staged_nodes(const SageVocabulary *voc) { return voc ? voc->n_staged : -1; }

extern "C" int sage_bow_transform(SageWorkspace *ws, const SageVocabulary *voc, const float *desc_dev, const int64_t *loc1d_dev,
                                  int M, int P, int32_t *word_ids_host, double *values_host, int capacity,
                                  int32_t *word_of_point_out_dev, SageBowStats *out)
{
  if (!ws || !voc || !desc_dev || !word_ids_host || !values_host || !out || M <= 0 || P < 1 || (!loc1d_dev && P != M) ||
      capacity < std::min(M, voc->n_words))
    return SAGE_E_INVALID;
  int rc;
  const size_t hit_words = (size_t)((voc->n_words + kBowScanTile - 1) / kBowScanTile) * kBowScanTile;
  if (ws->bow_hit.cap < hit_words * sizeof(uint32_t))
    ws->bow_hit_zero = false; // (a new allocation: nothing is known about it)
  if ((rc = ws->bow_hit.reserve(hit_words * sizeof(uint32_t))) ||
      (rc = ws->bow_host.reserve(offsetof(BowHost, ids) + (size_t)voc->n_words * sizeof(int32_t)))) // (every earlier call has been waited for)
    return rc;
  if (!ws->bow_hit_zero) // (a workspace's first call, a larger vocabulary, or the call before did not reach its compaction)
    SAGE_HIP(hipMemsetAsync(ws->bow_hit.p, 0, ws->bow_hit.cap, ws->stream));
  ws->bow_hit_zero = false; // (until this call's compact kernel has run)

  BowWalkParams W;
  W.desc = desc_dev; W.loc = loc1d_dev; W.P = P; W.M = M;
  W.voc_desc = voc->desc.as<float4>(); W.nodes = voc->nodes.as<BowNode>();
  W.C = voc->C; W.Cp4 = voc->Cp4; W.n_staged = voc->n_staged; W.depth = voc->depth;
  W.hit = ws->bow_hit.as<uint32_t>(); W.word_out = word_of_point_out_dev;
  const int nb = std::min((M + kBlock - 1) / kBlock, kBowMaxBlocks);
  hipLaunchKernelGGL(bow_walk_for(voc->C), dim3(nb), dim3(kBlock), voc->lds_bytes, ws->stream, W);
  BowHost *h = ws->bow_host.as<BowHost>();
  const unsigned epoch = ws_ticket_next(ws);
  hipLaunchKernelGGL(bow_compact_kernel, dim3(1), dim3(kBlock), 0, ws->stream, ws->bow_hit.as<uint32_t>(), voc->n_words, h,
                     &ws->hs()->ticket, epoch);
  SAGE_HIP(hipGetLastError());
  if ((rc = ws_ticket_await(ws, epoch)))
    return rc;
  ws->bow_hit_zero = true;

  // the finish: a function of the set of words reached
  const int n_hit = h->n_hit;
  if (n_hit < 0 || n_hit > std::min(M, voc->n_words))
    return SAGE_E_STATE; // (cannot happen: at most one word per point)
  std::vector<char> seen(voc->n_nodes, 0);
  int n_inner = 0, n_zero = 0, n_out = 0;
  double norm = 0.0;
  for (int k = 0; k < n_hit; ++k)
  {
    const int32_t w = h->ids[k];
    if (w < 0 || w >= voc->n_words)
      return SAGE_E_STATE; // (cannot happen: the flags beyond the vocabulary's words stay zero)
    for (int32_t b = voc->parent_bfs[voc->word_leaf[w]]; b >= 0 && !seen[b]; b = voc->parent_bfs[b])
    {
      seen[b] = 1;
      ++n_inner;
    }
    const double weight = voc->word_weight[w];
    if (!(weight > 0))
    {
      ++n_zero;
      continue;
    }
    const double value = weight * (double)M;
    word_ids_host[n_out] = w;
    values_host[n_out] = value;
    norm += std::fabs(value);
    ++n_out;
  }
  if (norm > 0.0)
    for (int k = 0; k < n_out; ++k)
      values_host[k] /= norm;
  out->n_points = M;
  out->n_words = n_out;
  out->n_leaves_hit = n_hit;
  out->n_zero_weight = n_zero;
  out->n_inner_nodes_hit = n_inner;
  return SAGE_OK;
}
