// window_plan.h -- the build-time policy of the window engine as pure integer arithmetic: which directed edges a rank owns,
// which of them are dense, whether a window uses the domain-decomposed solve, which rows of a keyframe's block the solver keeps,
// where a window's terms live, the run lengths of the two work lists.  Standard library only -- no HIP, no
// environment: the runtime applies its overrides to the results (window_build.hip), and tests/test_window_plan.py compiles
// this header with a host compiler.  An edge's length is its number of SUB-TILES (ceil(samples / kTile)) throughout.
#pragma once

#include <algorithm>
#include <vector>

namespace sage
{
namespace plan
{

// ---- ownership.  A link is two directed edges per factor type (a -> b, b -> a: global ids 2l, 2l + 1).  r05: rank r owns the
//      contiguous range [r*2n/world, (r+1)*2n/world) of the DIRECTED edges -- the two directions of a link may sit on two ranks
//      (both factor types of a direction stay together: the merged linearize pairs them).  With whole links, 42 links on 8 ranks
//      are 5 or 6 per rank, 20 % imbalance (BASELINE config 4: the 6-link ranks set the job's pace at 4.6x where the 5-link ranks
//      reach 6x); 84 directed edges are 10 or 11.  Links are added keyframe by keyframe, so a contiguous range touches
//      ~K/world + (back links) keyframes: only those need depth maps on this rank.  by_link: rank r owns the range
//      [r*n/world, (r+1)*n/world) of whole links instead (capi.shard_edges / capi.shard_links mirror the two rules).
struct Ownership
{
  std::vector<int> edges; // global directed edges of the rank, ascending
  std::vector<int> links; // links with at least one of them, ascending
};

inline Ownership owned_edges(int nlinks, int rank, int world, bool by_link)
{
  Ownership o;
  const long long nl = nlinks;
  if (by_link)
  {
    const int lo = (int)(nl * rank / world), hi = (int)(nl * (rank + 1) / world);
    for (int l = lo; l < hi; ++l)
    {
      o.edges.push_back(2 * l);
      o.edges.push_back(2 * l + 1);
    }
  }
  else
  {
    const int lo = (int)(2 * nl * rank / world), hi = (int)(2 * nl * (rank + 1) / world);
    for (int ge = lo; ge < hi; ++ge)
      o.edges.push_back(ge);
  }
  for (int ge : o.edges)
    if (o.links.empty() || o.links.back() != ge / 2)
      o.links.push_back(ge / 2);
  return o;
}

// which of a rank's owned directed edges carry the dense factors: those of links added with both factor types
// (link_is_dense[l] != 0); the others carry keypoint terms only -- no row of the dense edge tables, work lists or per-edge
// results.  The order of `owned` is kept: a dense edge's local index is its position in the answer.
inline std::vector<int> dense_edges(const std::vector<int> &owned, const std::vector<char> &link_is_dense)
{
  std::vector<int> out;
  for (int ge : owned)
    if (ge >= 0 && (size_t)(ge / 2) < link_is_dense.size() && link_is_dense[ge / 2])
      out.push_back(ge);
  return out;
}

// does the window use the domain-decomposed solve (shard_solve.cpp)?  Sharded windows only: on by request or for long windows,
// where the replicated factorisation of all K keyframes dominates the iteration (DESIGN s7: K = 512 on 8 ranks: 5x less solve).
// It derives its domains from whole links, so such a window also keeps the link granularity of the ownership.
// requested: the caller's parsed override -- < 0 none, 0 off, > 0 on
inline bool uses_domain_solve(int world, int K, int requested)
{
  return world > 1 && (requested >= 0 ? requested != 0 : K >= 256);
}

// ---- solver rows.  A keyframe's block has B = 7 + CS rows in three groups: pose 6, code CS, scale 1 (hold-mask bits 1, 2, 4:
//      sage_window_hold).  A group that EVERY keyframe of the window holds is left out of the damped system altogether: the
//      window then solves blocks of Bs < B rows, the kept groups in block order.  Holds inside a kept group stay rows of the
//      identity inside the smaller block (damped_system.h).  Nothing dropped, or everything: the window solves at B as ever.
struct SolverRows
{
  int B = 0, Bs = 0;          // rows of a keyframe's block / of its block in the solver
  int kept = 7;               // mask of the groups the solver keeps
  std::vector<int> to_block;  // [Bs] solver row -> block row
  std::vector<int> to_solver; // [B] block row -> solver row, -1: dropped
  bool compact() const { return Bs != B; }
};

inline SolverRows solver_rows(const unsigned char *hold, int K, int CS)
{
  const int first[3] = {0, 6, 6 + CS}, size[3] = {6, CS, 1};
  SolverRows s;
  s.B = 7 + CS;
  int all = K > 0 ? 7 : 0; // the groups every keyframe holds
  for (int k = 0; k < K; ++k)
    all &= hold ? hold[k] : 0;
  s.kept = (all == 7) ? 7 : (7 & ~all);
  s.to_solver.assign(s.B, -1);
  for (int grp = 0; grp < 3; ++grp)
    if (s.kept & (1 << grp))
      for (int r = first[grp]; r < first[grp] + size[grp]; ++r)
      {
        s.to_solver[r] = (int)s.to_block.size();
        s.to_block.push_back(r);
      }
  s.Bs = (int)s.to_block.size();
  return s;
}

// ---- terms.  A window's keypoint terms (kinds 0 / 1 / 2: reprojection, match geometry, loop-MG) and pose-graph terms (every
//      kind) put their AtA / Atb into the result buffers of a GROUP -- what a term's system looks like -- and their
//      {error, inliers} into one array.  AdjEntry::type of a term is 2 + group.
enum : int { kGroupPhoto = 0, kGroupGeo = 1, kGroupPoseScale = 2, kTermGroups = 3 };
constexpr int kKeypointKinds = 3;
// columns of a group's systems: the photometric edge's column map, the geometric edge's, poses and scales only
constexpr int term_group_dim(int group, int CS) { return group == kGroupPhoto ? 13 + CS : (group == kGroupGeo ? 14 + 2 * CS : 14); }
constexpr int keypoint_kind_group(int kind) { return kind; }
constexpr int graph_kind_group(int) { return kGroupPoseScale; }
constexpr int term_adj_type(int group) { return 2 + group; }

struct TermKey // a term as added: its kind, and whether this rank owns it (the runtime's rule)
{
  int kind;
  bool owned;
};
// where a term lives: its index in its family's device table (= launch position), its group, its index in the group's AtA / Atb
// buffers and in the {error, inliers} array; all -1 for a term of another rank
struct TermSlot
{
  int local = -1, group = -1, out = -1, stat = -1;
};
struct TermLayout
{
  std::vector<TermSlot> kp, graph;        // per term id (add order)
  std::vector<int> kp_order, graph_order; // launch order: term ids by `local`
  int count[kTermGroups] = {0, 0, 0};     // entries of each group's result buffers
  int n_keypoint() const { return (int)kp_order.size(); } // the keypoint kernel's terms = the leading entries of the stat array
  int n_graph() const { return (int)graph_order.size(); }
  int n_stats() const { return n_keypoint() + n_graph(); }
  int n_photo_stats() const { return count[kGroupPhoto]; } // leading stat entries (reprojection): the photometric total's
};

// both families in add order -> keypoint terms kind-major, each kind in add order, then the graph terms in add order: that is
// the stat array and the two launch orders; in a group's buffers the graph terms stand behind the loop-MG terms
inline TermLayout term_layout(const std::vector<TermKey> &kp, const std::vector<TermKey> &graph)
{
  TermLayout L;
  L.kp.assign(kp.size(), TermSlot());
  L.graph.assign(graph.size(), TermSlot());
  auto place = [&L](TermSlot &s, size_t id, std::vector<int> &order, int group) {
    s = TermSlot{(int)order.size(), group, L.count[group]++, L.n_stats()};
    order.push_back((int)id);
  };
  for (int kind = 0; kind < kKeypointKinds; ++kind)
    for (size_t i = 0; i < kp.size(); ++i)
      if (kp[i].kind == kind && kp[i].owned)
        place(L.kp[i], i, L.kp_order, keypoint_kind_group(kind));
  for (size_t i = 0; i < graph.size(); ++i)
    if (graph[i].owned)
      place(L.graph[i], i, L.graph_order, graph_kind_group(graph[i].kind));
  return L;
}

// ---- run lengths of the work lists
inline long long total_tiles(const std::vector<int> &tiles)
{
  long long total = 0;
  for (int t : tiles)
    total += t;
  return total;
}

// the typical edge: the median length (at least 1; 1 without edges)
inline int typical_edge(std::vector<int> tiles)
{
  if (tiles.empty())
    return 1;
  std::nth_element(tiles.begin(), tiles.begin() + tiles.size() / 2, tiles.end());
  return std::max(1, tiles[tiles.size() / 2]);
}

// geometric linearize: the two wave groups of a workgroup alternate over its sub-tiles (geo_kernels.hip), so a workgroup wants an
// even, longish run of them: the pipeline fill/drain costs one half-step per workgroup
// (r05, one rank's shard of the K = 64 window at world 8 = 2.9 k sub-tiles: runs of 8 leave 362 workgroups for 256 CUs --
//  85 us; runs of 4: 74 us, 2: 77 us; the full window's 23 k sub-tiles keep runs of 16)
inline int geo_run(long long total)
{
  return total >= 8192 ? 16 : (total >= 4096 ? 8 : (total >= 512 ? 4 : 2));
}

// photometric work list: the run length of a workgroup (sub-tiles it walks: prologue amortisation, vertical L1/L2 reuse between
// its bands).  Separate from it, the number of sub-tiles a workgroup accumulates in fp32 before a partial record goes out to the
// double sums (record_cadence below; MFMA chains of 64 fmaf per sub-tile and accumulator): the LM step's distance from the exact
// step grows with the chain length (K = 64 window, tests/tools/tpb_noise_probe.py: 8 -> 2.1e-4, 4 -> 1.2e-4, 2 -> 7.6e-5,
// 1 -> 4.9e-5 rel-L2; the fp32 oracle itself sits at 5.5e-5).  Records every 2 sub-tiles keep the step inside the 1e-4 parity bar.
inline int photo_run(const std::vector<int> &tiles, int FS)
{
  const long long total = total_tiles(tiles);
  const int T = typical_edge(tiles);
  // (r03, one rank's shard of the K = 64 window at world 8 / 4 = 2.9 k / 5.8 k sub-tiles: runs of 4 / 8 are 19 % / 8 % faster
  //  than the 1 / 2 the first heuristic picked; >= ~3 workgroups per CU stay in flight)
  int tpb = total >= 4096 ? 8 : (total >= 1536 ? 4 : (total >= 768 ? 2 : 1));
  // (r05, one rank's shard of BASELINE config 4 at world 8 -- FS = 32, 10 or 11 edges of 252 sub-tiles: with runs of 4 the
  //  11-edge shard's 693 workgroups take 0.231 ms where the 10-edge shard's 630 take 0.163; runs of 6: 0.187 / 0.163, runs
  //  of 7 / 9 / 12 worse for both.  At FS = 16 the same range wants runs of 4 (K = 64 shard: 0.084 ms; 5-8: 0.11-0.12))
  // (known oddity: for exactly those shards the multiple-of-8 pick below overrides the 6 -- 42 runs per edge; runs of 8 give 32)
  if (FS == 32 && total >= 1536 && total < 4096)
    tpb = 6;
  {
    // even runs: an edge of T sub-tiles is cut into ceil(T / tpb) workgroups of ceil(T / that) sub-tiles each -- with
    // T = 12 (3072 samples: the reference's default) runs of 8 leave a half-length second workgroup per edge and the
    // linearize 25 % slower than runs of 6 (BASELINE config 5: 1.85 -> 1.39 ms, error pass 0.49 -> 0.39 ms)
    const int nwg = (T + tpb - 1) / tpb, rem = T % tpb;
    if (rem != 0 && 4 * rem < 3 * tpb) // (a nearly full last run is left alone: T = 63 stays at runs of 8 -- 7 x 9 and
      tpb = (T + nwg - 1) / nwg;       //  9 x 7 measured 5-7 % slower on the headline window)
  }
  // r06 -- runs per edge a multiple of 8.  Workgroup b runs on XCD b % 8 and every XCD has its own L2: with 8 m runs per edge,
  // run j of EVERY edge lands on XCD j % 8 -- the same band of the image, whose destination texels the XCD's L2 then serves to
  // the next edges that share the keyframe.  The BASELINE sizes have it by luck (63 sub-tiles = 8 runs of 8, config 4: 32
  // runs); on the same window 13 / 11 / 7 runs per edge (SAGE_PHOTO_TPB = 5 / 6 / 10) cost the photometric linearize 20-30 %
  // and the error pass 50 % (profiles/r06_kernel_ab_experiments.txt s11).  Padding an edge to 8 m runs with empty work items
  // is no way out (the XCDs that get the real runs then carry twice the load: +60 %): the run LENGTH is chosen instead,
  // among lengths that leave a record cadence of 3-5 sub-tiles.
  // (r06, later: the edges that share a keyframe -- as destination or as source -- are TWO apart in the launch order, so a run
  //  count of 0 mod 4 already aligns them: taken when no candidate gives 0 mod 8 -- a 192 x 256 window, 165 sub-tiles per
  //  edge: runs of 8 = 21 per edge, runs of 6 = 28: linearize -18 %, error pass -27 %.  sage_window_tune_runs measures.)
  if (T >= 48 && ((T + tpb - 1) / tpb) % 8 != 0)
    for (int mod : {8, 4})
      for (int t : {8, 9, 10, 12, 6, 15, 16, 20})
        if (((T + t - 1) / t) % mod == 0)
          return t;
  return tpb;
}

// record cadence of a run length: a partial record every 3-5 sub-tiles (0 = one record per workgroup).  With the second level of
// the noise-critical tiles and their split accumulators in the kernel this puts the K = 64 LM step 7.0-8.2e-5 from the fp32
// oracle's on four windows (r03: tests/tools/delta_probe.py; one record per workgroup: 8.8-9.8e-5) for +2 % of the kernel
inline int record_cadence(int tpb)
{
  if (tpb < 6)
    return 0;
  return tpb % 4 == 0 ? 4 : (tpb % 5 == 0 ? 5 : (tpb % 3 == 0 ? 3 : 0)); // (r06: run lengths 6, 9, 10, 15)
}

// the run lengths sage_window_tune_runs times on a window: the rule's first, then the alternatives no longer than the typical edge
inline std::vector<int> tune_candidates(int rule, int typical)
{
  std::vector<int> cand{rule};
  for (int t : {4, 6, 8, 9, 10, 12, 16})
    if (t != rule && t <= typical && 2 * t >= std::min(rule, 8)) // (shorter than half the rule's runs: prologue-bound, not tried)
      cand.push_back(t);
  return cand;
}

} // namespace plan
} // namespace sage
