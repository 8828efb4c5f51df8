// voc_build.hip -- sage_vocabulary_build: the loop detector's vocabulary trained on the device (include/sage_ba.h, "training
// the vocabulary", states every rule; DBoW2's HKmeansStep / initiateClustersKMpp / setNodeWeights run one node at a time
// on the host with one blocking norm per (point, centre) pair).  Here a level's nodes are segments of the same launches:
//
//   vb_relayout_kernel     once: [C, M] channel-major -> padded point-major rows (16-byte loads), the identity order
//   vb_seed_init_kernel    per level, one workgroup per node: centre 0 from draw 0; a node of n <= k points is finished here
//   vb_seed_dist_kernel    per seeding round, one workgroup per (node, tile): min_d against the node's newest centre, the
//                          tile's fp64 sum
//   vb_seed_pick_kernel    per seeding round, one workgroup per node: the tiles' sums in tile order, the cut from the draw,
//                          the tile that reaches it, the position inside it; the picked point becomes the next centre
//   vb_lloyd_assign_kernel per Lloyd round, one workgroup per (unfinished node, tile): the node's centres in LDS, the
//                          assignment, the mismatches against the stored one, per cluster and channel the tile's fp64 sum
//   vb_lloyd_finish_kernel per Lloyd round, one workgroup per unfinished node: the tiles' sums in tile order -> the next
//                          centres; (mismatches, n, centres) to pinned memory; the last workgroup posts the ticket
//   vb_level_end_kernel    per level, one workgroup per node: the final centres and the clusters' sizes to pinned memory, per
//                          (tile, cluster) the offset of the stable partition
//   vb_scatter_kernel      per level, one workgroup per (node, tile): the order of the node's run, partitioned by child
//   vb_leaf_kernel, vb_doc_flag_kernel, vb_doc_count_kernel   at the end: the leaf of every point; Ni per word
// The host makes the stop / continue decisions (one ticket wait per Lloyd round), builds the work lists (finished nodes drop
// out) and keeps the tree.  No float atomics; no workgroup waits for another; every loop is bounded by n, k, C or the tiles.
#include "runtime_internal.h"
#include "sage_device.h"
#include "voc_build.h"

using namespace sage_voc;

namespace
{
struct VbNodeRec // pinned: one per node split at this level
{
  int32_t begin, n;       // its run of the order
  int32_t tile0, n_tiles; // n > k: its rows of the per-tile arrays
  int32_t cur;            // the centre set (0 / 1) that holds the centres to assign to
  int32_t pad;
  uint64_t hash;          // of its path: the draws
};
static_assert(sizeof(VbNodeRec) == 32, "sage_ba.h: pinned_bytes");

struct VbItem
{
  int32_t a, t; // node of the level, tile of the node
};

struct VbLevel // what every kernel of a level takes
{
  const VbNodeRec *recs; // [nA] pinned
  const VbItem *items;   // pinned
  const float4 *rows;    // [M][cp4]
  int32_t *ord, *ord2;   // [M]
  int32_t *cluster;      // [M] by position
  double *min_d;         // [M] by position
  float *centres;        // [2][A][k][Cp]
  int32_t *ncent;        // [A]
  double *tsum;          // [T][k][C]
  int32_t *tcnt, *toff;  // [T][k]
  int32_t *tmis;         // [T]
  double *tseed;         // [T]
  int4 *res;             // [A] pinned: (mismatches, n, centres, the node of this slot)
  int32_t *picks;        // [A][k] pinned
  int32_t *csize;        // [A][k] pinned
  float *centres_host;   // [A][k][Cp] pinned
  long long A;
  int k, C, cp4;
};

__device__ __forceinline__ float *vb_centre(const VbLevel &P, int set, int a, int c)
{
  return P.centres + (((size_t)set * P.A + a) * P.k + c) * (size_t)(4 * P.cp4);
}

template <int CP4T>
__device__ __forceinline__ void vb_load_row(float (&f)[CP4T * 4], const float4 *row, int cp4)
{
#pragma unroll
  for (int q = 0; q < CP4T; ++q)
  {
    const float4 v = q < cp4 ? row[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    f[4 * q + 0] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
  }
}

// sum_ch (f - c)^2: the expressions of bow.hip's bow_nearest, in its order (the walk must make the same decisions)
template <int CP4T>
__device__ __forceinline__ float vb_d2(const float (&f)[CP4T * 4], const float4 *c, int cp4)
{
  float d = 0.0f;
#pragma unroll
  for (int q = 0; q < CP4T; ++q)
    if (q < cp4)
    {
      const float4 v = c[q];
      const float e0 = f[4 * q + 0] - v.x, e1 = f[4 * q + 1] - v.y, e2 = f[4 * q + 2] - v.z, e3 = f[4 * q + 3] - v.w;
      d += e0 * e0;
      d += e1 * e1;
      d += e2 * e2;
      d += e3 * e3;
    }
  return d;
}

__global__ __launch_bounds__(kBlock) void vb_relayout_kernel(const float *desc, long long M, int C, int cp4, float4 *rows, int32_t *ord,
                                                             int32_t *ord2)
{
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= M)
    return;
  for (int q = 0; q < cp4; ++q)
  {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      v[j] = 4 * q + j < C ? desc[(long long)(4 * q + j) * M + i] : 0.0f;
    rows[i * cp4 + q] = make_float4(v[0], v[1], v[2], v[3]);
  }
  ord[i] = (int32_t)i;
  ord2[i] = (int32_t)i;
}

__global__ __launch_bounds__(kBlock) void vb_seed_init_kernel(const VbLevel P)
{
  const int a = blockIdx.x, tid = threadIdx.x;
  const VbNodeRec rec = P.recs[a];
  const int Cp = 4 * P.cp4;
  const float *rows = reinterpret_cast<const float *>(P.rows);
  if (rec.n <= P.k) // one child per point
  {
    for (int q = tid; q < rec.n * Cp; q += kBlock)
      vb_centre(P, 0, a, q / Cp)[q % Cp] = rows[(size_t)P.ord[rec.begin + q / Cp] * Cp + q % Cp];
    if (tid < rec.n)
      P.cluster[rec.begin + tid] = tid;
    if (tid == 0)
      P.ncent[a] = rec.n;
    return;
  }
  long long idx = (long long)(vb_unit(vb_draw(rec.hash, 0)) * (double)rec.n);
  idx = idx < rec.n - 1 ? idx : rec.n - 1;
  if (tid < Cp)
    vb_centre(P, 0, a, 0)[tid] = rows[(size_t)P.ord[rec.begin + idx] * Cp + tid];
  if (tid == 0)
  {
    P.ncent[a] = 1;
    P.picks[(size_t)a * P.k] = (int32_t)idx;
  }
}

template <int CP4T>
__global__ __launch_bounds__(kBlock) void vb_seed_dist_kernel(const VbLevel P, int r)
{
  __shared__ __attribute__((aligned(16))) float s_c[kVbMaxC];
  __shared__ double s_w[kBlock / 64];
  const VbItem it = P.items[blockIdx.x];
  const VbNodeRec rec = P.recs[it.a];
  if (P.ncent[it.a] != r) // this node's seeding has ended
    return;
  const int tid = threadIdx.x, Cp = 4 * P.cp4;
  if (tid < Cp)
    s_c[tid] = vb_centre(P, 0, it.a, r - 1)[tid];
  __syncthreads();
  const int p = it.t * kVbTile + tid;
  double md = 0.0;
  if (p < rec.n)
  {
    const int pos = rec.begin + p;
    const double old = r == 1 ? 0.0 : P.min_d[pos];
    md = old;
    if (r == 1 || old > 0.0)
    {
      float f[CP4T * 4];
      vb_load_row<CP4T>(f, P.rows + (size_t)P.ord[pos] * P.cp4, P.cp4);
      const double dist = (double)sqrtf(vb_d2<CP4T>(f, reinterpret_cast<const float4 *>(s_c), P.cp4));
      md = (r == 1 || dist < old) ? dist : old;
      P.min_d[pos] = md;
    }
  }
  // the pairwise tree: lanes l and l + s for s = 1 .. 32 inside a wave, then 64 and 128 across the waves
  double v = md;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1)
    v += __shfl_down(v, s, 64);
  if ((tid & 63) == 0)
    s_w[tid >> 6] = v;
  __syncthreads();
  if (tid == 0)
    P.tseed[rec.tile0 + it.t] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

__global__ __launch_bounds__(kBlock) void vb_seed_pick_kernel(const VbLevel P, int r)
{
  __shared__ double s_v[kVbTile];
  __shared__ double s_total, s_before;
  __shared__ int s_tile, s_idx;
  const int a = blockIdx.x, tid = threadIdx.x;
  const VbNodeRec rec = P.recs[a];
  if (rec.n <= P.k || P.ncent[a] != r)
    return;
  const double *ts = P.tseed + rec.tile0;
  // pass 1: the tiles' sums in tile order
  double run = 0.0; // (thread 0's)
  for (int base = 0; base < rec.n_tiles; base += kVbTile)
  {
    const int m = min(kVbTile, rec.n_tiles - base);
    if (tid < m)
      s_v[tid] = ts[base + tid];
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < m; ++i)
        run += s_v[i];
    __syncthreads();
  }
  if (tid == 0)
    s_total = run;
  __syncthreads();
  const double total = s_total;
  if (!(total > 0.0)) // dist_sum == 0: fewer than k centres
  {
    if (tid == 0)
      P.picks[(size_t)a * P.k + r] = -1;
    return;
  }
  double cut = total;
  for (int at = 0; at < 64; ++at) // the do-while of the redraw
  {
    const double c = vb_unit(vb_draw(rec.hash, r + at * P.k)) * total;
    if (c != 0.0)
    {
      cut = c;
      break;
    }
  }
  // pass 2: the first tile whose running sum reaches the cut (the last tile's running sum IS the total, and cut <= total)
  if (tid == 0)
  {
    s_tile = rec.n_tiles - 1;
    s_before = 0.0;
  }
  run = 0.0;
  bool found = false; // (thread 0's)
  for (int base = 0; base < rec.n_tiles; base += kVbTile)
  {
    const int m = min(kVbTile, rec.n_tiles - base);
    if (tid < m)
      s_v[tid] = ts[base + tid];
    __syncthreads();
    if (tid == 0 && !found)
      for (int i = 0; i < m; ++i)
      {
        const double next = run + s_v[i];
        if (next >= cut)
        {
          s_tile = base + i;
          s_before = run;
          found = true;
          break;
        }
        run = next;
      }
    __syncthreads();
  }
  const int tile = s_tile;
  // inside the tile: position by position from the running sum before it
  const int p = tile * kVbTile + tid;
  s_v[tid] = p < rec.n ? P.min_d[rec.begin + p] : 0.0;
  __syncthreads();
  if (tid == 0)
  {
    double s = s_before;
    int pick = -1, last_pos = 0;
    const int m = min(kVbTile, rec.n - tile * kVbTile);
    for (int i = 0; i < m; ++i)
    {
      s += s_v[i];
      if (s_v[i] > 0.0)
        last_pos = i;
      if (s >= cut)
      {
        pick = i;
        break;
      }
    }
    s_idx = tile * kVbTile + (pick >= 0 ? pick : last_pos);
  }
  __syncthreads();
  const int idx = s_idx, Cp = 4 * P.cp4;
  if (tid < Cp)
    vb_centre(P, 0, a, r)[tid] = reinterpret_cast<const float *>(P.rows)[(size_t)P.ord[rec.begin + idx] * Cp + tid];
  if (tid == 0)
  {
    P.ncent[a] = r + 1;
    P.picks[(size_t)a * P.k + r] = idx;
  }
}

// dynamic LDS: the node's centres [nc][Cp] | the tile's rows [256][Cp + 4] (the padding keeps the 16-byte row stores of a
// wave on different banks) | the tile's clusters [256]
template <int CP4T>
__global__ __launch_bounds__(kBlock) void vb_lloyd_assign_kernel(const VbLevel P)
{
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];
  __shared__ int s_w[kBlock / 64];
  const VbItem it = P.items[blockIdx.x];
  const VbNodeRec rec = P.recs[it.a];
  const int tid = threadIdx.x, Cp = 4 * P.cp4, stride = Cp + 4;
  const int nc = P.ncent[it.a];
  float *s_c = s_dyn;
  float *s_rows = s_dyn + (size_t)P.k * Cp;
  int *s_assign = reinterpret_cast<int *>(s_rows + (size_t)kVbTile * stride);
  {
    const float *g = vb_centre(P, rec.cur, it.a, 0);
    for (int i = tid; i < nc * Cp; i += kBlock)
      s_c[i] = g[i];
  }
  __syncthreads();
  const int p = it.t * kVbTile + tid;
  int best = -1, mis = 0;
  if (p < rec.n)
  {
    const int pos = rec.begin + p;
    float f[CP4T * 4];
    vb_load_row<CP4T>(f, P.rows + (size_t)P.ord[pos] * P.cp4, P.cp4);
    float best_d = 0.0f;
    for (int c = 0; c < nc; ++c)
    {
      const float d = vb_d2<CP4T>(f, reinterpret_cast<const float4 *>(s_c + (size_t)c * Cp), P.cp4);
      if (c == 0 || d < best_d) // the first smallest wins
      {
        best_d = d;
        best = c;
      }
    }
    mis = P.cluster[pos] != best;
    P.cluster[pos] = best;
    float4 *dst = reinterpret_cast<float4 *>(s_rows + (size_t)tid * stride);
#pragma unroll
    for (int q = 0; q < CP4T; ++q)
      if (q < P.cp4)
        dst[q] = make_float4(f[4 * q + 0], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
  }
  s_assign[tid] = best;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    mis += __shfl_down(mis, s, 64);
  if ((tid & 63) == 0)
    s_w[tid >> 6] = mis;
  __syncthreads();
  const size_t tile = (size_t)rec.tile0 + it.t;
  if (tid == 0)
    P.tmis[tile] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
  // per (cluster, channel): the tile's points in ascending position
  const int m = min(kVbTile, rec.n - it.t * kVbTile);
  for (int q = tid; q < nc * P.C; q += kBlock)
  {
    const int c = q / P.C, ch = q - c * P.C;
    double acc = 0.0;
    int cnt = 0;
    for (int i = 0; i < m; ++i)
      if (s_assign[i] == c)
      {
        acc += (double)s_rows[(size_t)i * stride + ch];
        ++cnt;
      }
    P.tsum[(tile * P.k + c) * P.C + ch] = acc;
    if (ch == 0)
      P.tcnt[tile * P.k + c] = cnt;
  }
}

__global__ __launch_bounds__(kBlock) void vb_lloyd_finish_kernel(const VbLevel P, unsigned *done, volatile unsigned *ticket, unsigned epoch)
{
  __shared__ int s_w[kBlock / 64];
  const int tid = threadIdx.x;
  const int a = P.res[blockIdx.x].w;
  const VbNodeRec rec = P.recs[a];
  const int nc = P.ncent[a], Cp = 4 * P.cp4;
  const float *cur = vb_centre(P, rec.cur, a, 0);
  float *next = vb_centre(P, rec.cur ^ 1, a, 0);
  for (int q = tid; q < nc * Cp; q += kBlock)
  {
    const int c = q / Cp, ch = q - c * Cp;
    float out = 0.0f; // (the padding channels)
    if (ch < P.C)
    {
      double acc = 0.0;
      long long cnt = 0;
      for (int t = 0; t < rec.n_tiles; ++t) // tile order
      {
        const size_t tile = (size_t)rec.tile0 + t;
        acc += P.tsum[(tile * P.k + c) * P.C + ch];
        cnt += P.tcnt[tile * P.k + c];
      }
      out = cnt > 0 ? (float)(acc / (double)cnt) : cur[q]; // an emptied cluster keeps its centre
    }
    next[q] = out;
  }
  int mis = 0;
  for (int t = tid; t < rec.n_tiles; t += kBlock)
    mis += P.tmis[rec.tile0 + t];
#pragma unroll
  for (int s = 32; s > 0; s >>= 1)
    mis += __shfl_down(mis, s, 64);
  if ((tid & 63) == 0)
    s_w[tid >> 6] = mis;
  __syncthreads();
  if (tid == 0)
  {
    int4 *slot = P.res + blockIdx.x;
    slot->x = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    slot->y = rec.n;
    slot->z = nc;
    __threadfence_system(); // the result is on its way before this workgroup is counted as done
    if (atomicAdd(done, 1u) == gridDim.x - 1u)
    {
      *done = 0; // (the next launch comes after this kernel)
      __threadfence_system();
      *ticket = epoch;
    }
  }
}

__global__ __launch_bounds__(kBlock) void vb_level_end_kernel(const VbLevel P)
{
  __shared__ int s_size[kVbMaxK], s_first[kVbMaxK];
  const int a = blockIdx.x, tid = threadIdx.x;
  const VbNodeRec rec = P.recs[a];
  const int nc = P.ncent[a], Cp = 4 * P.cp4;
  const float *cur = vb_centre(P, rec.cur, a, 0);
  float *out = P.centres_host + (size_t)a * P.k * Cp;
  for (int q = tid; q < nc * Cp; q += kBlock)
    out[q] = cur[q];
  if (rec.n <= P.k) // one point per child: nothing to partition
  {
    if (tid < P.k)
      P.csize[(size_t)a * P.k + tid] = tid < nc ? 1 : -1; // (-1: no such child)
    return;
  }
  if (tid < P.k)
  {
    int size = 0;
    if (tid < nc)
      for (int t = 0; t < rec.n_tiles; ++t)
        size += P.tcnt[((size_t)rec.tile0 + t) * P.k + tid];
    s_size[tid] = size;
    P.csize[(size_t)a * P.k + tid] = tid < nc ? size : -1;
  }
  __syncthreads();
  if (tid == 0)
  {
    int at = 0;
    for (int c = 0; c < nc; ++c)
    {
      s_first[c] = at;
      at += s_size[c];
    }
  }
  __syncthreads();
  if (tid < nc)
  {
    int at = s_first[tid];
    for (int t = 0; t < rec.n_tiles; ++t)
    {
      const size_t i = ((size_t)rec.tile0 + t) * P.k + tid;
      P.toff[i] = at;
      at += P.tcnt[i];
    }
  }
}

__global__ __launch_bounds__(kBlock) void vb_scatter_kernel(const VbLevel P)
{
  __shared__ int s_assign[kVbTile];
  const VbItem it = P.items[blockIdx.x];
  const VbNodeRec rec = P.recs[it.a];
  const int tid = threadIdx.x, p = it.t * kVbTile + tid;
  const int c = p < rec.n ? P.cluster[rec.begin + p] : -1;
  s_assign[tid] = c;
  __syncthreads();
  if (c < 0)
    return;
  int rank = 0; // the points of the tile before this one in the same cluster: the partition is stable
  for (int i = 0; i < tid; ++i)
    rank += s_assign[i] == c;
  const int to = P.toff[((size_t)rec.tile0 + it.t) * P.k + c] + rank;
  if (to >= 0 && to < rec.n) // (always)
    P.ord2[rec.begin + to] = P.ord[rec.begin + p];
}

// runs: the leaves that hold points, ascending by begin; every position lies in exactly one
__global__ __launch_bounds__(kBlock) void vb_leaf_kernel(const int32_t *ord, long long M, const int32_t *run_begin, const int32_t *run_id,
                                                         int n_runs, int32_t *leaf)
{
  const long long pos = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (pos >= M)
    return;
  int lo = 0, hi = n_runs - 1; // the last run with begin <= pos
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (run_begin[mid] <= pos)
      lo = mid;
    else
      hi = mid - 1;
  }
  leaf[ord[pos]] = run_id[lo];
}

// flags [d1 - d0][n_words] bytes: document d reaches word w (an idempotent store); the points of documents d0 .. d1 - 1
__global__ __launch_bounds__(kBlock) void vb_doc_flag_kernel(const int32_t *word, const int64_t *doc_begin, int d0, int d1, int n_words,
                                                             unsigned char *flags)
{
  const long long i = doc_begin[d0] + (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= doc_begin[d1])
    return;
  int lo = d0, hi = d1 - 1; // the last document with begin <= i (empty documents share a begin: the last of them holds i)
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (doc_begin[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  const int w = word[i];
  if (w >= 0 && w < n_words)
    flags[(size_t)(lo - d0) * n_words + w] = 1;
}

__global__ __launch_bounds__(kBlock) void vb_doc_count_kernel(const unsigned char *flags, int n_docs_chunk, int n_words, int32_t *ni)
{
  const int w = blockIdx.x * kBlock + threadIdx.x;
  if (w >= n_words)
    return;
  int s = 0;
  for (int d = 0; d < n_docs_chunk; ++d)
    s += flags[(size_t)d * n_words + w];
  ni[w] += s;
}

struct VbKernels
{
  void (*dist)(const VbLevel, int);
  void (*assign)(const VbLevel);
};
VbKernels vb_kernels_for(int cp4)
{
  if (cp4 <= 4)
    return {vb_seed_dist_kernel<4>, vb_lloyd_assign_kernel<4>};
  if (cp4 <= 8)
    return {vb_seed_dist_kernel<8>, vb_lloyd_assign_kernel<8>};
  return {vb_seed_dist_kernel<16>, vb_lloyd_assign_kernel<16>};
}
} // namespace

struct SageVocabularyBuild
{
  SageVocabularyBuildConfig cfg{};
  int C = 0, n_docs = 0;
  long long M = 0;
  std::vector<int32_t> parent, word_id, ni;
  std::vector<float> descriptors;
  std::vector<double> weight;
  SageVocabularyBuildStats stats{};
  DevBuf leaf; // [M]
};

extern "C" void sage_vocabulary_build_destroy(SageVocabularyBuild *b) { delete b; }

extern "C" int sage_vocabulary_build_desc(const SageVocabularyBuild *b, SageVocabularyDesc *d)
{
  if (!b || !d)
    return SAGE_E_INVALID;
  d->n_nodes = (int32_t)b->parent.size();
  d->C = b->C;
  d->parent = b->parent.data();
  d->descriptors = b->descriptors.data();
  d->weight = b->weight.data();
  d->word_id = b->word_id.data();
  d->scoring = b->cfg.scoring;
  return SAGE_OK;
}

extern "C" int sage_vocabulary_build_docs_with_word(const SageVocabularyBuild *b, const int32_t **ni, int *n_words)
{
  if (!b || !ni || !n_words)
    return SAGE_E_INVALID;
  *ni = b->ni.data();
  *n_words = (int)b->ni.size();
  return SAGE_OK;
}

extern "C" int sage_vocabulary_build_node_of_point(const SageVocabularyBuild *b, const int32_t **leaf_node_dev)
{
  if (!b || !leaf_node_dev)
    return SAGE_E_INVALID;
  *leaf_node_dev = b->leaf.as<int32_t>();
  return SAGE_OK;
}

extern "C" int sage_vocabulary_build_stats(const SageVocabularyBuild *b, SageVocabularyBuildStats *stats)
{
  if (!b || !stats)
    return SAGE_E_INVALID;
  *stats = b->stats;
  return SAGE_OK;
}

namespace
{
struct VbScratch // everything but the leaves goes with the call
{
  DevBuf rows, min_d, ord, ord2, cluster, word, centres, ncent, tsum, tcnt, toff, tmis, tseed, ni, done, flags, doc_begin;
  PinnedBuf recs, items, res, picks, csize, centres_host;
};

int vb_run(SageWorkspace *ws, SageVocabularyBuild *b, const float *desc_dev, const int64_t *doc_begin, const VbPlan &pl)
{
  const int k = b->cfg.k, L = b->cfg.L, C = b->C, Cp = pl.Cp, cp4 = pl.Cp / 4;
  const long long M = b->M, A = pl.A, T = pl.T;
  hipStream_t s = ws->stream;
  VbScratch S;
  int rc;
  if ((rc = S.rows.reserve((size_t)M * Cp * 4)) || (rc = S.min_d.reserve((size_t)M * 8)) || (rc = S.ord.reserve((size_t)M * 4)) ||
      (rc = S.ord2.reserve((size_t)M * 4)) || (rc = S.cluster.reserve((size_t)M * 4)) || (rc = b->leaf.reserve((size_t)M * 4)) ||
      (rc = S.word.reserve((size_t)M * 4)) || (rc = S.centres.reserve((size_t)8 * A * k * Cp)) || (rc = S.ncent.reserve((size_t)4 * A)) ||
      (rc = S.tsum.reserve((size_t)T * 8 * k * C)) || (rc = S.tcnt.reserve((size_t)T * 4 * k)) || (rc = S.toff.reserve((size_t)T * 4 * k)) ||
      (rc = S.tmis.reserve((size_t)T * 4)) || (rc = S.tseed.reserve((size_t)T * 8)) || (rc = S.ni.reserve((size_t)4 * pl.W)) ||
      (rc = S.done.reserve(16)) || (rc = S.flags.reserve((size_t)kVbFlagBytes)) ||
      (rc = S.doc_begin.reserve((size_t)(b->n_docs + 1) * 8)) || // (+ 8 (n_docs + 1) bytes: not a function of the plan's arguments)
      (rc = S.recs.reserve((size_t)32 * A)) || (rc = S.items.reserve((size_t)8 * T)) || (rc = S.res.reserve((size_t)16 * A)) ||
      (rc = S.picks.reserve((size_t)4 * A * k)) || (rc = S.csize.reserve((size_t)4 * A * k)) ||
      (rc = S.centres_host.reserve((size_t)4 * A * k * Cp)))
    return rc;
  SAGE_HIP(hipMemsetAsync(S.done.p, 0, 16, s));
  SAGE_HIP(hipMemsetAsync(S.ni.p, 0, (size_t)4 * pl.W, s));
  SAGE_HIP(hipMemcpyAsync(S.doc_begin.p, doc_begin, (size_t)(b->n_docs + 1) * 8, hipMemcpyHostToDevice, s));

  VbLevel P;
  P.recs = S.recs.as<VbNodeRec>(); P.items = S.items.as<VbItem>(); P.rows = S.rows.as<float4>();
  P.ord = S.ord.as<int32_t>(); P.ord2 = S.ord2.as<int32_t>(); P.cluster = S.cluster.as<int32_t>(); P.min_d = S.min_d.as<double>();
  P.centres = S.centres.as<float>(); P.ncent = S.ncent.as<int32_t>(); P.tsum = S.tsum.as<double>(); P.tcnt = S.tcnt.as<int32_t>();
  P.toff = S.toff.as<int32_t>(); P.tmis = S.tmis.as<int32_t>(); P.tseed = S.tseed.as<double>(); P.res = S.res.as<int4>();
  P.picks = S.picks.as<int32_t>(); P.csize = S.csize.as<int32_t>(); P.centres_host = S.centres_host.as<float>();
  P.A = A; P.k = k; P.C = C; P.cp4 = cp4;
  VbNodeRec *recs = S.recs.as<VbNodeRec>();
  VbItem *items = S.items.as<VbItem>();
  int4 *res = S.res.as<int4>();
  const VbKernels K = vb_kernels_for(cp4);
  const size_t assign_lds = ((size_t)k * Cp + (size_t)kVbTile * (Cp + 4)) * sizeof(float) + kVbTile * sizeof(int);
  if (assign_lds > 48 * 1024)
    SAGE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(K.assign), hipFuncAttributeMaxDynamicSharedMemorySize, (int)assign_lds));

  const unsigned nbM = (unsigned)((M + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(vb_relayout_kernel, dim3(nbM), dim3(kBlock), 0, s, desc_dev, M, C, cp4, S.rows.as<float4>(), P.ord, P.ord2);
  SAGE_HIP(hipGetLastError());

  std::vector<VbRawNode> raw(1);
  raw[0].n = M;
  raw[0].hash = vb_path_hash(b->cfg.seed, nullptr, 0);
  std::vector<float> raw_desc((size_t)C, 0.0f); // [raw node][C]; the root's row is zero
  std::vector<int32_t> active(1, 0), live, next_active;
  SageVocabularyBuildStats &st = b->stats;
  for (int level = 1; level <= L && !active.empty(); ++level)
  {
    const int li = level - 1, nA = (int)active.size();
    if ((long long)nA > A)
      return SAGE_E_STATE; // (cannot happen: sage_ba.h, A)
    int n_km = 0, n_tiles = 0, launches = 0, waits = 0;
    for (int a = 0; a < nA; ++a)
    {
      const VbRawNode &nd = raw[active[a]];
      VbNodeRec &r = recs[a];
      r.begin = (int32_t)nd.begin; r.n = (int32_t)nd.n; r.cur = 0; r.pad = 0; r.hash = nd.hash;
      r.tile0 = n_tiles; r.n_tiles = 0;
      if (nd.n > k)
      {
        r.n_tiles = (int32_t)((nd.n + kVbTile - 1) / kVbTile);
        n_tiles += r.n_tiles;
        ++n_km;
      }
    }
    if ((long long)n_tiles > T)
      return SAGE_E_STATE; // (cannot happen: sage_ba.h, T)
    auto list_items = [&](const std::vector<int32_t> &nodes) {
      int n = 0;
      for (int32_t a : nodes)
        for (int t = 0; t < recs[a].n_tiles; ++t)
          items[n++] = VbItem{a, t};
      return n;
    };
    live.clear();
    for (int a = 0; a < nA; ++a)
      if (recs[a].n_tiles > 0)
        live.push_back(a);
    const int n_items_all = list_items(live);
    hipLaunchKernelGGL(vb_seed_init_kernel, dim3(nA), dim3(kBlock), 0, s, P);
    ++launches;
    if (n_km > 0)
      for (int r = 1; r < k; ++r)
      {
        hipLaunchKernelGGL(K.dist, dim3(n_items_all), dim3(kBlock), 0, s, P, r);
        hipLaunchKernelGGL(vb_seed_pick_kernel, dim3(nA), dim3(kBlock), 0, s, P, r);
        launches += 2;
      }
    SAGE_HIP(hipGetLastError());
    int round = 0;
    while (!live.empty())
    {
      ++round;
      const int n_items = round == 1 ? n_items_all : list_items(live);
      for (size_t i = 0; i < live.size(); ++i)
        res[i] = make_int4(0, 0, 0, live[i]);
      const unsigned epoch = ws_ticket_next(ws);
      hipLaunchKernelGGL(K.assign, dim3(n_items), dim3(kBlock), assign_lds, s, P);
      hipLaunchKernelGGL(vb_lloyd_finish_kernel, dim3((unsigned)live.size()), dim3(kBlock), 0, s, P, S.done.as<unsigned>(), &ws->hs()->ticket,
                         epoch);
      SAGE_HIP(hipGetLastError());
      launches += 2;
      if ((rc = ws_ticket_await(ws, epoch)))
        return rc;
      ++waits;
      size_t kept = 0;
      for (size_t i = 0; i < live.size(); ++i)
      {
        const int32_t a = live[i];
        const int mismatch = res[i].x, n = res[i].y;
        if (n != recs[a].n)
          return SAGE_E_STATE; // (cannot happen: the slot was written by its workgroup)
        const float rate = (float)mismatch / (float)n;
        const bool stop = round >= 2 && (double)rate < 1.0e-3;
        const bool capped = !stop && b->cfg.max_iterations > 0 && round >= b->cfg.max_iterations;
        if (capped)
          ++st.nodes_capped;
        if (stop || capped)
          continue;
        recs[a].cur ^= 1; // the means become the centres of the next round
        live[kept++] = a;
      }
      live.resize(kept);
    }
    // the level's end: centres and sizes out, the stable partition
    for (int a = 0, n = 0; a < nA; ++a) // (the scatter takes every tile of the level again)
      for (int t = 0; t < recs[a].n_tiles; ++t)
        items[n++] = VbItem{a, t};
    hipLaunchKernelGGL(vb_level_end_kernel, dim3(nA), dim3(kBlock), 0, s, P);
    ++launches;
    if (n_km > 0)
    {
      hipLaunchKernelGGL(vb_scatter_kernel, dim3(n_items_all), dim3(kBlock), 0, s, P);
      ++launches;
      SAGE_HIP(hipMemcpyAsync(P.ord, P.ord2, (size_t)M * 4, hipMemcpyDeviceToDevice, s));
    }
    SAGE_HIP(hipGetLastError());
    if ((rc = ws_ticket_wait(ws)))
      return rc;
    ++launches; // (the ticket's)
    ++waits;
    next_active.clear();
    for (int a = 0; a < nA; ++a)
    {
      const int32_t r = active[a];
      const long long n = raw[r].n;
      int nc = 0;
      long long total = 0;
      for (int c = 0; c < k && P.csize[(size_t)a * k + c] >= 0; ++c) // (fewer than k: n <= k, or the seeding ended early)
      {
        total += P.csize[(size_t)a * k + c];
        ++nc;
      }
      if (total != n || nc < 1)
        return SAGE_E_STATE; // (cannot happen: every point is in one cluster)
      raw[r].first_child = (int32_t)raw.size();
      raw[r].n_children = nc;
      long long at = raw[r].begin;
      for (int c = 0; c < nc; ++c)
      {
        VbRawNode ch;
        ch.parent = r; ch.child_index = c; ch.level = level; ch.begin = at; ch.n = P.csize[(size_t)a * k + c];
        ch.hash = vb_child_hash(raw[r].hash, c);
        at += ch.n;
        if (level < L && ch.n > 1)
          next_active.push_back((int32_t)raw.size());
        raw.push_back(ch);
        const float *src = P.centres_host + ((size_t)a * k + c) * Cp;
        raw_desc.insert(raw_desc.end(), src, src + C);
      }
    }
    st.nodes[li] = nA; st.kmeans_nodes[li] = n_km; st.seed_rounds[li] = n_km > 0 ? k - 1 : 0; st.rounds[li] = round;
    st.launches[li] = launches; st.waits[li] = waits;
    st.levels = level;
    active.swap(next_active);
  }

  // DBoW2's numbering, the words, the arrays of the result
  std::vector<int32_t> id_of_raw, order;
  vb_number(raw, id_of_raw, order);
  const int n_nodes = (int)raw.size();
  b->parent.assign(n_nodes, -1);
  b->word_id.assign(n_nodes, -1);
  b->weight.assign(n_nodes, 0.0);
  b->descriptors.assign((size_t)n_nodes * C, 0.0f);
  int n_words = 0;
  std::vector<int32_t> word_node; // node id of every word
  for (int id = 0; id < n_nodes; ++id)
  {
    const VbRawNode &nd = raw[order[id]];
    b->parent[id] = nd.parent < 0 ? -1 : id_of_raw[nd.parent];
    std::memcpy(&b->descriptors[(size_t)id * C], &raw_desc[(size_t)order[id] * C], (size_t)C * sizeof(float));
    if (id > 0 && nd.n_children == 0)
    {
      b->word_id[id] = n_words++;
      word_node.push_back(id);
    }
  }
  st.n_nodes = n_nodes;
  st.n_words = n_words;
  b->ni.assign(n_words, 0);
  if ((long long)n_words > pl.W)
    return SAGE_E_STATE; // (cannot happen: at most k^L leaves)

  // the leaf of every point: the runs of the leaves that hold points, ascending (raw order within a level is by begin; sort)
  {
    std::vector<std::pair<int32_t, int32_t>> runs;
    for (int r = 1; r < n_nodes; ++r)
      if (raw[r].n_children == 0 && raw[r].n > 0)
        runs.emplace_back((int32_t)raw[r].begin, id_of_raw[r]);
    std::sort(runs.begin(), runs.end());
    std::vector<int32_t> flat(2 * runs.size());
    for (size_t i = 0; i < runs.size(); ++i)
    {
      flat[i] = runs[i].first;
      flat[runs.size() + i] = runs[i].second;
    }
    if ((long long)runs.size() > M || runs.empty())
      return SAGE_E_STATE; // (cannot happen: the runs partition [0, M))
    int32_t *tab = S.min_d.as<int32_t>(); // (the seeding is over: 8 bytes per run fit)
    SAGE_HIP(hipMemcpyAsync(tab, flat.data(), flat.size() * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(vb_leaf_kernel, dim3(nbM), dim3(kBlock), 0, s, P.ord, M, tab, tab + runs.size(), (int)runs.size(),
                       b->leaf.as<int32_t>());
    SAGE_HIP(hipGetLastError());
    SAGE_HIP(hipStreamSynchronize(s)); // (`flat` goes out of scope)
  }

  // the weights: Ni through the library's own walk
  if (b->cfg.weighting == SAGE_VOC_TF_IDF || b->cfg.weighting == SAGE_VOC_IDF)
  {
    SageVocabularyDesc d;
    sage_vocabulary_build_desc(b, &d);
    d.scoring = SAGE_BOW_L1; // (the walk does not depend on it)
    SageVocabulary *voc = nullptr;
    if ((rc = sage_vocabulary_create(&d, &voc)))
      return rc;
    const int cap = (int)std::min<long long>(M, n_words);
    std::vector<int32_t> ids(cap);
    std::vector<double> vals(cap);
    SageBowStats bs;
    rc = sage_bow_transform(ws, voc, desc_dev, nullptr, (int)M, (int)M, ids.data(), vals.data(), cap, S.word.as<int32_t>(), &bs);
    sage_vocabulary_destroy(voc);
    if (rc)
      return rc;
    long long flag_bytes = kVbFlagBytes;
    if (const char *env = std::getenv("SAGE_VOC_FLAG_BYTES")) // tests: several chunks of documents at small sizes
      flag_bytes = std::max(0LL, std::min(flag_bytes, std::atoll(env)));
    const int chunk = (int)std::max<long long>(1, flag_bytes / n_words); // documents per pass: at least one (n_words <= 2^20 bytes)
    const int64_t *db = S.doc_begin.as<int64_t>();
    for (int d0 = 0; d0 < b->n_docs; d0 += chunk)
    {
      const int d1 = std::min(b->n_docs, d0 + chunk);
      const long long pts = doc_begin[d1] - doc_begin[d0];
      if (pts <= 0)
        continue;
      SAGE_HIP(hipMemsetAsync(S.flags.p, 0, (size_t)(d1 - d0) * n_words, s));
      hipLaunchKernelGGL(vb_doc_flag_kernel, dim3((unsigned)((pts + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, S.word.as<int32_t>(), db, d0, d1,
                         n_words, S.flags.as<unsigned char>());
      hipLaunchKernelGGL(vb_doc_count_kernel, dim3((unsigned)((n_words + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                         S.flags.as<unsigned char>(), d1 - d0, n_words, S.ni.as<int32_t>());
    }
    SAGE_HIP(hipGetLastError());
    SAGE_HIP(hipMemcpyAsync(b->ni.data(), S.ni.p, (size_t)n_words * 4, hipMemcpyDeviceToHost, s));
    SAGE_HIP(hipStreamSynchronize(s));
  }
  std::vector<double> w;
  vb_weights(b->cfg.weighting, b->n_docs, b->ni, w);
  for (int i = 0; i < n_words; ++i)
    b->weight[word_node[i]] = w[i];
  return SAGE_OK;
}
} // namespace

extern "C" int sage_vocabulary_build(SageWorkspace *ws, const SageVocabularyBuildConfig *cfg, const float *desc_dev, int C, int64_t M,
                                     const int64_t *doc_begin_host, int n_docs, SageVocabularyBuild **out)
{
  if (!ws || !cfg || !desc_dev || !doc_begin_host || !out || n_docs < 1 || cfg->max_iterations < 0 ||
      cfg->weighting < SAGE_VOC_TF_IDF || cfg->weighting > SAGE_VOC_BINARY || cfg->scoring < SAGE_BOW_L1 ||
      cfg->scoring > SAGE_BOW_DOT_PRODUCT)
    return SAGE_E_INVALID;
  VbPlan pl;
  int rc = vb_plan(C, M, cfg->k, cfg->L, &pl);
  if (rc == SAGE_E_INVALID)
    return rc;
  if (doc_begin_host[0] != 0 || doc_begin_host[n_docs] != M)
    return SAGE_E_INVALID;
  for (int d = 0; d < n_docs; ++d)
    if (doc_begin_host[d + 1] < doc_begin_host[d])
      return SAGE_E_INVALID;
  if (rc)
    return rc;
  SageVocabularyBuild *b = new SageVocabularyBuild();
  b->cfg = *cfg;
  b->C = C;
  b->M = M;
  b->n_docs = n_docs;
  rc = vb_run(ws, b, desc_dev, doc_begin_host, pl);
  if (rc)
  {
    (void)hipStreamSynchronize(ws->stream); // (nothing of the call's scratch is in use when it is freed)
    delete b;
    return rc;
  }
  *out = b;
  return SAGE_OK;
}
