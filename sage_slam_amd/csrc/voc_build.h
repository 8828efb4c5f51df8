// voc_build.h -- what the two halves of sage_vocabulary_build share (include/sage_ba.h, "training the vocabulary"):
//   voc_build.hip       the device side and the level loop
//   voc_build_host.cpp  (no HIP) the draw function, the argument checks, the plan, DBoW2's numbering, the weights from Ni
#pragma once

#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SAGE_VB_HD __host__ __device__
#else
#define SAGE_VB_HD
#endif

namespace sage_voc
{
constexpr int kVbTile = 256;                  // positions of a node per work item (one per lane)
constexpr int kVbMaxC = 64, kVbMaxK = 64, kVbMaxL = 8;
constexpr long long kVbMaxWords = 1 << 20;
constexpr long long kVbFlagBytes = 1 << 24;   // the document counts' flags: one byte per (document of the chunk, word)
constexpr unsigned long long kVbGamma = 0x9E3779B97F4A7C15ull;

SAGE_VB_HD inline uint64_t vb_mix(uint64_t z) // splitmix64's finalizer
{
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the hash of a node's path, and draw j from it: sage_vocabulary_build_draw = vb_draw(vb_path_hash(...), j)
inline uint64_t vb_path_hash(uint64_t seed, const int32_t *path, int depth)
{
  uint64_t h = vb_mix(seed + kVbGamma);
  for (int i = 0; i < depth; ++i)
    h = vb_mix((h ^ (uint64_t)path[i]) + kVbGamma);
  return h;
}
SAGE_VB_HD inline uint64_t vb_child_hash(uint64_t h, int child) { return vb_mix((h ^ (uint64_t)child) + kVbGamma); }
SAGE_VB_HD inline uint64_t vb_draw(uint64_t h, int j) { return vb_mix(h + (uint64_t)(j + 1) * kVbGamma); }
SAGE_VB_HD inline double vb_unit(uint64_t draw) { return (double)(draw >> 11) * (1.0 / 9007199254740992.0); } // 2^-53

// sizes of everything a build allocates (sage_ba.h states the formulas; elements, not bytes, unless named so)
struct VbPlan
{
  int Cp = 0;
  long long W = 0, A = 0, T = 0; // words at most, nodes split at one level at most, tiles of one level's k-means nodes at most
  long long device_bytes = 0, pinned_bytes = 0;
};
int vb_check_shape(int C, long long M, int k, int L); // SAGE_OK, SAGE_E_INVALID, SAGE_E_UNSUPPORTED
int vb_plan(int C, long long M, int k, int L, VbPlan *p);

// the tree as the level loop makes it: nodes in the order of their creation level by level
struct VbRawNode
{
  int32_t parent = -1;      // raw index; -1: the root
  int32_t child_index = 0;  // among its parent's children
  int32_t level = 0;
  int32_t first_child = -1; // raw index of child 0 (children are consecutive); -1: a leaf
  int32_t n_children = 0;
  long long begin = 0, n = 0; // its run of the order, its points
  uint64_t hash = 0;          // vb_path_hash of its path
};
// DBoW2's creation order: id_of_raw[r] = the node id of raw node r; order[id] = r
void vb_number(const std::vector<VbRawNode> &raw, std::vector<int32_t> &id_of_raw, std::vector<int32_t> &order);
// log((double)n_docs / (double)Ni) per word, 0 where Ni == 0; TF / BINARY: 1
void vb_weights(int weighting, int n_docs, const std::vector<int32_t> &ni, std::vector<double> &w);
} // namespace sage_voc
