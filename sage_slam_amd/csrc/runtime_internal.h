// runtime_internal.h -- shared by the host-runtime translation units behind the C ABI (include/sage_ba.h):
//   operators.hip       workspaces (work-list cache, ticket wait), the per-edge operator API (df::*_calculate mirrors): an
//                       enqueue function per family + the public wrappers that wait; the producer entry points
//   tracker.hip         tracker wiring of the LM callbacks (sage_track_frame): one evaluation over the enqueue functions; B
//                       problems in lock-step (sage_track_frame_batch): one round over the batched launches
//   overlap.hip         overlap statistics of a tracked pose (sage_track_overlap): its kernels and the host finish
//   depth_scale.hip     the mapper's depth-scale correction and device medians (sage_depth_scale_ratio, sage_median_f32):
//                       the per-point kernel and the exact radix selection; B rows of either in the launches of one
//   depth_scale_host.cpp  (no HIP) the layout of such a batch
//   loop_accept_host.cpp  (no HIP) sage_loop_accept's rules: accept test, pose hand-over, sort, redundancy filter
//   bow.hip             the loop detector's bag of words (sage_vocabulary_*, sage_bow_transform): the vocabulary's device
//                       layout, the tree walk, the compaction of the words reached, the host finish
//   bow_database.cpp    (no HIP) the L1 score of two bag-of-words vectors and the inverted-file database
//   voc_build.hip       training the vocabulary (sage_vocabulary_build): the level loop, the seeding and Lloyd rounds of all
//                       nodes of a level, the stable partition by child, the document counts
//   voc_build_host.cpp  (no HIP) its draws, argument checks, plan, DBoW2's node numbering, the weights from the document counts
//   registration.hip    robust registration of keypoint matches (sage_robust_registration, sage_match_points): the pair
//                       kernel, the endpoint sort, the scan fused with the vote's cost and argmin, the hand-over; the loop
//                       detector's pre-check of B candidates (sage_loop_precheck), a host composition
//   match_batch.hip     one query descriptor map against B candidate maps (sage_cycle_match_batch): the sliced match kernel,
//                       the merge of the slices' winners, flags and counts
//   registration_host.cpp  (no HIP) the scalar TLS vote and the finish of the solve: chain TIMs, GNC-TLS rotation, translation
//   window.hip          a finalized window's accessors, keyframe variables in and out, helpers the window units share
//   window_eval.hip     evaluating the factors at a variable set: linearize + assembly, error pass (the window's big kernels)
//   window_reduce.hip   sums over ranks (hook, peer emulation), the pinned totals mirror and its waits, the total error
//   window_solve.hip    from a system to a candidate: priors, damped solve, separator solve, accept / reset / variable exchange
//   window_lm.hip       the LM iteration: one policy around three sequences (classic, schur, at_candidate)
//   window_dogleg.hip   the dogleg iteration: A g, A n and the dots on the device, trial points as blends, the step
//   dogleg_host.cpp     (no HIP) the dogleg point, gtsam's trust-region policy around a callback, the incidence lists
//   window_profile.hip  optional kernel timing of a window: event pool, per-kernel event pairs, phase marks
//   window_build.hip    building a window: create / add / finalize (stages; policy in window_plan.h), run plan and its tuning
//   keyframe_prepare.hip  prepared keyframes (sage_keyframe_prepare_batch): stages 3-5 of finalize for B keyframes outside any
//                       window, its two batch kernels, the handle's reference count
//   keyframe_prepare_host.cpp  (no HIP) the configuration fingerprint, the checks, the layouts and the plan (keyframe_prepare.h)
//   window_terms.hip    keypoint and pose-graph terms: add / get, their finalize stage, their two launches
//   window_dist.hip     sharded windows: NUMA placement, all-reduce hook, native RCCL binding
//   window_factors.hip  f2: per-Values factor cache behind the gtsam adapter (prepass, factor blocks, NearestPsd)
//   window_relin.hip    partial relinearization: the stale edges of a linearize, their compacted launch plan (its kernel), the
//                       depth maps' stamps, the relinearization marks and the masked accept
//   window_prior.hip    marginal priors on a window: add / get, their finalize stage, the evaluation and add kernels' launches,
//                       sage_window_marginalize (the sub-system of the dropped keyframes' factors, summed on the host)
//   marginal_host.cpp   (no HIP) the Schur complement, the prior's handle, the host mirror of the term, the layout plan's C view
//   relin_host.cpp      (no HIP) the reads table and gtsam's relinearization check (relin_plan.h), stateless
//   factor_blocks.cpp   (no HIP) what a cached factor is: shape, projection of its own matrix, cut into HessianFactor blocks
//   tsdf.hip            TSDF fusion of depth maps into a voxel volume (sage_tsdf_*): the volume, the per-view kernel, all views
//                       in one pass over the volume (bricks in registers, views staged in LDS, the conservative cull)
//   tsdf_host.cpp       (no HIP) the frustum bounds, the volume's plan, the calls' argument checks
//   window_tsdf.hip     a window's keyframes into a volume (sage_window_fuse_tsdf), the depth range of its maps
// window_state.h holds the parts SageWindow is made of (host variables, dense factor side, term side, factor cache, totals
// mirror, distributed state, profiler); device_buffers.h holds the owners of device and pinned allocations (DevBuf, PinnedBuf: also
// included by solve_kernels.hip); the layouts of the workspace's pinned regions (WsHostStats, TrackHost) are below
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <sched.h>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include <dlfcn.h>
// RCCL: types only -- the library is bound at run time with dlopen (sage_rccl_*), hosts without it never load it, and a
// build host without the RCCL headers still compiles (the handful of types the binding needs are declared here then)
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C"
{
  typedef struct ncclComm *ncclComm_t;
  typedef struct
  {
    char internal[128];
  } ncclUniqueId;
  typedef enum { ncclSuccess = 0 } ncclResult_t;
  typedef enum { ncclSum = 0 } ncclRedOp_t;
  typedef enum { ncclDouble = 8 } ncclDataType_t; // nccl.h: ncclFloat64 = ncclDouble = 8
}
#endif

#include "device_buffers.h" // DevBuf, PinnedBuf
#include "host_math.h"
#include "factor_blocks.h" // FactorShape and the functions over it
#include "host_threads.h" // placement, shutdown (the window units do not touch the block solver itself)
#include "sage_ba.h"
#include "sage_internal.h"
#include "keypoint_batch.h"
#include "graph_batch.h"
#include "window_plan.h" // SolverRows, TermLayout
#include "registration_plan.h" // RegBatchPlan
#include "depth_scale_plan.h"  // SelBatchPlan
#include "loop_accept.h"       // sage_loop_accept's host rules
#include "dogleg.h"            // the dogleg step's dots, partial slots and pinned record
#include "keyframe_prepare.h"  // a prepared keyframe's fingerprint, layout and plan; the handle itself
#include "marginal.h"          // a marginal prior's handle, the layout of a window's prior terms
#include "covariance.h"        // the closed pattern and the recursion of the marginal covariances
#include "tsdf.h"              // a TSDF volume's brick shapes, the view checks

using namespace sage;

#define SAGE_HIP(expr)                \
  do                                  \
  {                                   \
    hipError_t _e = (expr);           \
    if (_e != hipSuccess)             \
      return (int)_e;                 \
  } while (0)

namespace sage_rt
{

inline int pick_tiles_per_block(long long total_tiles)
{
  // keep >= ~4 workgroups per CU in flight while amortising the partial write (one per workgroup)
  if (total_tiles >= 8192)
    return 4;
  if (total_tiles >= 4096)
    return 2;
  return 1;
}

// host-built work list for a set of edges with per-edge pixel counts
struct WorkList
{
  std::vector<WorkItem> work;
  std::vector<int32_t> edge_first, edge_tiles; // per edge: first work item, number of work items
  std::vector<int32_t> rec_first, rec_count;   // per edge: first partial record, number of partial records
  int tiles_per_block = 1;
  int flush = 1; // sub-tiles per partial record (== tiles_per_block unless the photometric linearize asks for less)
  int n_records = 0;
  // `order`: optional sequence of the edges (a permutation of 0..N.size()-1) the work items are laid out in; every
  // edge's items stay contiguous
  void build(const std::vector<int> &N, int tpb_override = 0, const std::vector<int> *order = nullptr, int flush_ = 0)
  {
    long long total = 0;
    for (int n : N)
      total += (n + kTile - 1) / kTile;
    tiles_per_block = tpb_override > 0 ? tpb_override : pick_tiles_per_block(total);
    flush = (flush_ > 0 && flush_ < tiles_per_block && tiles_per_block % flush_ == 0) ? flush_ : tiles_per_block;
    work.clear();
    edge_first.assign(N.size(), 0);
    edge_tiles.assign(N.size(), 0);
    rec_first.assign(N.size(), 0);
    rec_count.assign(N.size(), 0);
    n_records = 0;
    for (size_t i = 0; i < N.size(); ++i)
    {
      const size_t e = order ? (size_t)(*order)[i] : i;
      const int tiles = (N[e] + kTile - 1) / kTile;
      edge_first[e] = (int32_t)work.size();
      for (int t = 0; t < tiles; t += tiles_per_block)
        work.push_back(WorkItem{(int32_t)e, t});
      edge_tiles[e] = (int32_t)work.size() - edge_first[e];
      rec_first[e] = n_records;
      rec_count[e] = (tiles + flush - 1) / flush;
      n_records += rec_count[e];
    }
  }
};

// spin until done() holds (a ticket a kernel posts into pinned memory), looking at the clock every 1024 spins; false: 0.05 s
// have passed and done() still does not hold -- the caller waits the ordinary way
template <class Pred>
inline bool spin_until(Pred done)
{
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (!done())
  {
    __builtin_ia32_pause();
    if ((++spins & 0x3ff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.05)
      return false;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return true;
}

} // namespace sage_rt
using namespace sage_rt;

// =====================================================================================================
// workspace
// =====================================================================================================
// the workspace's pinned regions as the device sees them; the kernels write them over PCIe themselves (no device-to-host
// copy afterwards)
struct WsHostStats // SageWorkspace::host_stats
{
  float stats[4]; // the operator's {error, inliers}, written by its kernels
  float pad[4];
  unsigned ticket; // ws_ticket_wait
  unsigned tail[7];
};
static_assert(offsetof(WsHostStats, ticket) == 8 * sizeof(float) && sizeof(WsHostStats) == 16 * sizeof(float), "device-visible layout");

struct TrackHost // SageWorkspace::trk_host: one tracker evaluation (tracker.hip)
{
  float pose[12]; // what the kernels read: R [9], t [3]
  float pad[4];
  float photo_AtA[49], photo_Atb[7];
  float kp_AtA[49], kp_Atb[7];
  float stats[4]; // {error, inliers} of the photometric term, then of the keypoint term
  float tail[12];
};
static_assert(offsetof(TrackHost, photo_AtA) == 16 * sizeof(float) && offsetof(TrackHost, photo_Atb) == (16 + 49) * sizeof(float) &&
                  offsetof(TrackHost, kp_AtA) == (16 + 56) * sizeof(float) && offsetof(TrackHost, kp_Atb) == (16 + 56 + 49) * sizeof(float) &&
                  offsetof(TrackHost, stats) == (16 + 112) * sizeof(float) && sizeof(TrackHost) == (16 + 112 + 4 + 12) * sizeof(float),
              "device-visible layout");

enum class WorkKind { none, dense, tracker }; // dense: pick_tiles_per_block's run length; tracker: one kTile per workgroup

// depth_sigma.hip: what a depth-sigma launch reads besides the keyframes' planes -- the items' table and their fp32 (code,
// scale) covariances, built in pinned memory and copied to the device on the launch's stream.  `copied` says the copy of the
// last call has left the pinned side: the next call waits for that (not for the kernel) before it writes there again
struct DepthSigmaStage
{
  PinnedBuf host;
  DevBuf dev;
  hipEvent_t copied = nullptr;
  bool busy = false;
  DepthSigmaStage() = default;
  DepthSigmaStage(const DepthSigmaStage &) = delete;
  DepthSigmaStage &operator=(const DepthSigmaStage &) = delete;
  ~DepthSigmaStage()
  {
    if (copied)
      (void)hipEventDestroy(copied);
  }
};
struct DepthSigmaEntry // one keyframe of a launch; S: HOST, the (CS + 1) x (CS + 1) block with leading dimension ldS
{
  const float *bias, *basis, *code, *scale_dev; // scale_dev: where the scale lies on the device, or null: `scale`
  float scale;
  const double *S;
  size_t ldS;
  float *out;
};
// one launch for n > 0 keyframes on stream s; arguments are the caller's to check (CS 16 or 32, mode 0 / 1, H * W >= 1).
// before / after: optional events recorded right around the kernel (sage_window_depth_sigma_timing)
int depth_sigma_enqueue(hipStream_t s, DepthSigmaStage &stage, const DepthSigmaEntry *e, int n, int H, int W, int CS, int mode,
                        hipEvent_t before = nullptr, hipEvent_t after = nullptr);

struct SageWorkspace
{
  hipStream_t stream = nullptr;
  DepthSigmaStage sigma; // sage_depth_sigma_batch
  DevBuf work, edge_first, edge_tiles, partials, misc, dpt0;
  PinnedBuf host_stats; // WsHostStats, from sage_workspace_create on
  unsigned ticket_epoch = 0;
  // the one-edge work list `work` / `edge_first` / `edge_tiles` hold (ws_bind_work)
  WorkKind list_kind = WorkKind::none;
  int list_N = 0;
  int n_work = 0;
  int tiles_per_block = 1;
  // tracker wiring (sage_track_frame): one evaluation = several operator launches that write their results into trk_host,
  // then one ticket.  Buffers persist across frames.
  DevBuf trk_dpts, trk_kp_dpts; // dof 7: depths scaled for the evaluation
  PinnedBuf trk_host;           // TrackHost, from the first tracked frame on; [B] of them from a batch of B on
  // batched tracker (sage_track_frame_batch): the call's pinned tables (TrackBatchProblem [B] | KpTrackProblem [B] | the
  // rounds' request lists | the round's scale items | the rounds' work items), the problems' partial records, and (dof 7)
  // the round's scaled depths: per problem its samples' [N], then its keypoints' [NK]
  PinnedBuf trk_table;
  DevBuf trk_bpart, trk_bdpts;
  // overlap statistics (sage_track_overlap, overlap.hip): per-workgroup partials + survivor counters, the survivors of
  // both hull sets, and the pinned region the finish kernel publishes into; all grow with M and go with the workspace
  // A batch (sage_track_overlap_batch) holds B rows in the same three; ov_batch_launches: what the last batch launched
  DevBuf ov_part, ov_surv;
  PinnedBuf ov_host; // [header [B] | survivors of the input set [M][2] | of the warped set [M][2], per row]
  int ov_batch_launches = 0;
  // exact selection (sage_depth_scale_ratio, sage_median_f32: depth_scale.hip): the keys [M] (grow with M), the histograms,
  // counts and hand-over state of the passes, and the pinned record the finish kernel publishes
  DevBuf sel_keys, sel_scratch;
  PinnedBuf sel_host;
  bool sel_scratch_zero = false; // the last call's finish kernel has run: the scratch is zero again
  // A batch (sage_depth_scale_ratio_batch, sage_median_f32_batch) holds B rows in the same three: the keys of all rows, a
  // scratch and a pinned record per row; sel_scratch_zero speaks of the whole scratch allocation.  sel_batch_launches:
  // what the last batch launched
  int sel_batch_launches = 0;
  // bag of words (sage_bow_transform, bow.hip): one flag per word of the vocabulary (rounded up to the compaction's tile),
  // and the pinned record the compact kernel publishes: [count, pad x 3 | the word ids reached, ascending]
  DevBuf bow_hit;
  PinnedBuf bow_host;
  bool bow_hit_zero = false; // the last call's compact kernel has run: every flag is zero again
  // robust registration (sage_robust_registration, sage_match_points: registration.hip): the endpoints' keys and payloads [P],
  // the pairs' measurements (X, r) [pairs], the scan's per-tile sums, offsets and minima with the two counters, and the
  // pinned record the last kernel publishes (RegHost; also where sage_match_points leaves its count and mean).  All grow
  // with N and go with the workspace.  A batch (sage_robust_registration_batch) holds all its voting problems in the same
  // five: segments of the first three, per-segment rows of the fourth, one record per problem in the fifth;
  // sage_match_points_batch leaves [B] counts and means there.  reg_batch_launches: what the last batch launched
  DevBuf reg_keys, reg_payload, reg_pairs, reg_tiles;
  PinnedBuf reg_host;
  int reg_batch_launches = 0;
  // where the solves' finish runs (sage_workspace_set_registration_finish): SAGE_REG_FINISH_HOST, or _DEVICE: reg_finish_kernel
  // behind the vote, its records behind the votes' in reg_host
  int reg_finish_mode = 0;
  // batched cycle match (sage_cycle_match_batch: match_batch.hip): the slices' (response, pixel) pairs of both passes
  // [2][B][S][K], the counter of finished workgroups (zero between calls), the pinned counts [SAGE_MATCH_MAX_BATCH]; the
  // device's CU count (0: not asked yet) and the number of slices of the last call
  DevBuf mb_part, mb_done;
  PinnedBuf mb_host;
  int mb_cus = 0, mb_slices = 0;
  // loop pre-check (sage_loop_precheck: registration.hip): the way back [B][K], then the B candidates' gathered points
  DevBuf pre_scratch;
  // batched projection (sage_factor_psd_batch: psd_project.hip): the matrices' pinned records [n]; what the last call launched
  PinnedBuf psd_host;
  int psd_launches = 0;
  // prepared keyframes (sage_keyframe_prepare_batch: keyframe_prepare.hip): the call's tables, mark planes, status and tile
  // counts (PrepScratch, keyframe_prepare.h); what the last call launched
  DevBuf prep_scratch;
  int prep_launches = 0;
  // TSDF fusion (sage_tsdf_integrate_batch: tsdf.hip): the views' table, built in pinned memory and copied to the device on
  // the launch's stream (the staging protocol of the sigma launch)
  DepthSigmaStage tsdf_stage;

  WsHostStats *hs() const { return host_stats.as<WsHostStats>(); }
  TrackHost *trk() const { return trk_host.as<TrackHost>(); }
};

// a TSDF volume (tsdf.hip): its arrays, the per-brick counts of the last batch and what that batch was
struct SageTsdfVolume
{
  SageWorkspace *ws = nullptr;
  SageTsdfPlan plan{};
  DevBuf tsdf, weight, color; // [voxels] each; color only with plan.with_color
  DevBuf kept;                // [bricks of the smallest brick shape] int32: views the brick kept in the last batch
  hipEvent_t order = nullptr; // orders the workspace's stream and a caller's (sage_window_fuse_tsdf)
  int last_views = 0, last_brick_x = 0; // the last batch: 0 views = none yet
};
// sage_tsdf_integrate_batch on stream s (arguments checked by the caller: tsdf::check_batch); s != the volume's stream: s waits
// for what the volume's stream holds, and the volume's stream for the launch
int tsdf_integrate_batch_on(SageTsdfVolume *vol, hipStream_t s, const SageTsdfView *views, int n, int flags);

// operators.hip
// enqueue a one-lane kernel that posts a ticket behind everything in the workspace's stream and spin until it shows up
// (instead of a blocking hipStreamSynchronize)
int ws_ticket_wait(SageWorkspace *ws);
// the two halves of it, for an operator whose last kernel posts the ticket itself (into hs()->ticket, behind a
// __threadfence_system()): the epoch to post, and the spin until it shows up
unsigned ws_ticket_next(SageWorkspace *ws);
int ws_ticket_await(SageWorkspace *ws, unsigned epoch);
// the tracker's operators, enqueued only: they validate, reserve and launch; the kernels write {error, inliers} to `stats`
// and nobody waits.  The public entry points are these with the workspace's own stats slot, then a ticket wait
int track_photo_enqueue(SageWorkspace *ws, bool jac, int dof, float *AtA, float *Atb, float *stats, const float *R,
                        const float *t, const float *mask1, const float *dpts0, const float *homo, const float *feat0s,
                        const float *feat1, const float *grad1, const SagePyramid *pyr, float scale0, float eps,
                        const float *weights_dev, int N, int FS);
int track_reproj_enqueue(SageWorkspace *ws, bool jac, float *AtA, float *Atb, float *stats, const float *R, const float *t,
                         const float *sampled_dpts0, const float *homo, const float *matched_2d, const SageCamera *cam,
                         float eps, float loss_param, float weight, int N);
int track_match_geom_enqueue(SageWorkspace *ws, int mode, bool jac, float *AtA, float *Atb, float *stats, const float *R,
                             const float *t, const float *sampled_dpts0, const float *matched_dpts1, const float *homo0,
                             const float *matched_homo1, float scale0, float loss_param, float weight, int N);

// psd_project.hip: the batched Higham projection of n > 0 matrices of D columns, one launch on `s`, nobody waits; stats [n]
// is device-visible memory (device or pinned)
int psd_project_enqueue(hipStream_t s, int D, int n, const float *AtA_dev, double *C_dev, SagePsdStats *stats);

// registration_host.cpp: SAGE_OK, SAGE_E_INVALID or SAGE_E_UNSUPPORTED for a parameter set
int registration_check_params(const SageRegistrationParams *p);

// instantiated (CS, FS) combinations of the factor kernels
static inline bool supported(int CS, int FS)
{
  return (CS == 16 || CS == 32) && (FS == 16 || FS == 32);
}

// ---- window engine ----
namespace sage
{
struct AdjEntry // one (edge, role) incidence of a keyframe
{
  int32_t type; // 0 photo, 1 geo; a term: plan::term_adj_type(its group)
  int32_t edge; // local edge index; a term: its index in the group's result buffers
  int32_t role; // 0: keyframe is the edge's source ("0"), 1: destination ("1")
};

struct LinkEdges // local edge indices of a link, -1 if the link is not owned by this rank
{
  int32_t e_ab, e_ba; // same indices for photo and geo tables
};

struct AssembleParams
{
  const float *AtA_p, *Atb_p, *stats_p; // photo per-edge results
  const float *AtA_g, *Atb_g, *stats_g;
  const double *wide_p, *wide_g; // optional: per-edge [D*D + D] results before their fp32 rounding (EdgeOut::wide)
  const int32_t *adj_start; // [K+1]
  const AdjEntry *adj;
  const LinkEdges *links; // [nlinks]
  double *packed;
  double *tail_mirror; // pinned host copy of the 4-double tail (single-rank windows), or null
  int K, nlinks, CS, n_edges_p, n_edges_g;
  int split;               // > 1: every output block is shared by `split` consecutive workgroups (small workgroups)
  const int32_t *blocks;   // optional: the output blocks to assemble (ids 0..K-1 keyframes, K..K+nlinks-1 links, K+nlinks tail)
  // keypoint and graph terms (zero without them): per link the terms on its two directions (AdjEntry::role = direction),
  // and their results
  const int32_t *link_terms_start; // [nlinks+1]
  const AdjEntry *link_terms;
  TermResults terms;
};

struct ErrorTotalsSide
{
  const int32_t *edge_first, *edge_tiles;
  const float *partials; // [n_work][2]
  float *stats;          // [n_edges][2]
  float fallback, scale;
  int n_edges;           // 0: factor type unused
  int stride, err_off, cnt_off; // record layout: floats per workgroup record, slots of the error sum / the inlier count
};

} // namespace sage

#include "window_state.h"

// a prepared keyframe (keyframe_prepare.hip): stages 3-5 of sage_window_finalize for one keyframe, done once.  Immutable once
// sage_keyframe_prepare_batch has returned, refs apart: windows on any stream or host thread of its device read it
struct SagePreparedKeyframe
{
  std::atomic<int> refs{1};        // the caller's reference + one per window that holds it; the last release frees
  sage::prep::Fingerprint fp;      // what it was prepared under: a window takes it only under the same
  SageKeyframeView view;           // the caller's arrays, borrowed (N: the caller's samples)
  int slots = 0;                   // what a window's kernels walk: N, or 64 x tiles (padded)
  int ordered = 0, padded = 0;     // ordered 0: a pixel sampled twice -- loc / homo below are the caller's
  sage::prep::Layout lay;
  DevBuf mem;                      // planes | locations | rays | pre-sampled source features (lay)
  const float *pk = nullptr;       // [3 (f, gx, gy)][FS/4][P][4]
  const int64_t *loc = nullptr;    // [slots]
  const float *homo = nullptr;     // [slots][3]
  const float *f0s = nullptr;      // negated, [L][FS/4][slots][4]
};
void prepared_retain(SagePreparedKeyframe *pk);
void prepared_release(SagePreparedKeyframe *pk); // (sage_keyframe_release)

struct SageWindow
{
  SageWindowConfig cfg;
  hipStream_t stream = nullptr;
  bool finalized = false;
  int rank = 0, world = 1;
  int K = 0, B = 0, VS = 0; // VS: floats per keyframe in the device variable array
  std::vector<SageKeyframeView> views;
  std::vector<SagePreparedKeyframe *> prepared; // per keyframe: the handle it was added by (a reference held), or null: a view
  std::vector<const float *> kf_pk, kf_f0s;     // (finalize) per keyframe: its relaid planes and pre-sampled source features,
                                                // the window's own (pk, f0s below) or its handle's
  SageWindowBuildStats build_stats{};           // stages 3-5 of the last finalize
  HostVars hv;                      // host variables of both sets, their initial values
  std::vector<float> link_geo_loss; // per link: the geometric factors' Cauchy parameter, 0 = cfg.geo_loss_param
  std::vector<std::pair<int, int>> links; // (a, b) with a < b
  std::vector<char> link_dense;           // per link: 1 = carries the dense factors (sage_window_add_link), 0 = keypoint
                                          // terms only (sage_window_add_keypoint_link)
  std::vector<uint8_t> hold;              // per keyframe: mask of held variables (sage_window_hold), empty = none
  sage::plan::SolverRows rows;            // (finalize) the rows of a keyframe's block the solver keeps: window_plan.h
  std::vector<int> local_links;           // indices into links (links with at least one local directed edge)
  std::vector<int> owned_edges;           // this rank's directed edges, global ids 2 * link + direction, ascending: whose
                                          // keypoint terms it evaluates
  std::vector<int> local_edges;           // ... those of them that carry dense factors (plan::dense_edges; local edge index
                                          // = position in this list; a single-rank window of dense links: the identity)
  int n_edges = 0;                        // local DENSE directed edges per factor type
  // device
  DevBuf vars[2];                       // [K][VS]: pose 12, scale 1, code CS
  DevBuf sorted_loc, sorted_homo;       // raster-ordered copies of the keyframes' sampled locations
  std::vector<std::pair<const int64_t *, const float *>> user_samples; // the caller's arrays
  std::vector<int> user_n; // ... and their lengths (views[k].N becomes the tile-padded slot count for keyframes relaid with holes)
  DevBuf dpt, dgrad, depth_items[2];    // per-keyframe depth maps of the set being evaluated
  int n_depth = 0;                      // keyframes this rank's edges touch (= entries of depth_items)
  int dpt_set = -1;                     // variable set the depth maps currently hold (-1: none) ...
  bool dgrad_valid = false;             // ... and whether their gradients are up to date as well
  DevBuf geo_px;                        // merged linearize: per local edge and source pixel {omega, D, dD/dx, dD/dy} (geo -> photo)
  bool merge_ok = false;                // both factor types on, geometric weight > 0, not switched off (SAGE_NO_MERGE)
  DevBuf pk;                            // engine-internal channel-group pyramids [K][3 (f,gx,gy)][FS/4][P][4]
  DevBuf f0s;                           // per keyframe: pre-sampled source features, negated [L][FS/4][N][4]
  DenseSide dense[2];                   // [kPhoto], [kGeo]: edge tables, work list, partials, per-edge results
  PhotoRecordPlan photo_rec;            // the photometric linearize's partial records
  std::vector<int> Nedge;               // samples (slots) per local directed edge: what the photometric run plan is built from
  int tpb_heur = 1;                     // run length the static rule chose (sage_window_tune_runs measures alternatives)
  DevBuf adj_start, adj, link_edges, packed, errbuf;
  TotalsMirror mirror;                  // pinned totals + tickets; written by the kernels only if kernels_mirror_totals()
  WindowDist dist;                      // all-reduce hook, shard plan, peer emulation, this rank's share of `packed`
  std::vector<double> host_packed;
  std::vector<double> delta;
  // device solver (solve_kernels.hip); nullptr -> duplicate links: host block solve (sage_block_solve).  After a device solve the candidate's host mirrors are refreshed lazily (sync_candidate).
  sage::DeviceSolver *solver = nullptr;
  bool cand_pending = false;
  double residuals_per_lin = 0, bytes_per_lin = 0;
  bool have_lin = false;
  // linearize-at-candidate LM (SageLmConfig::linearize_at_candidate): which variables the packed system belongs to
  uint64_t vars_epoch = 1, lin_epoch = 0; // lin_epoch == vars_epoch: `packed` is the linearisation at the current variables
  bool spec_err_valid = false;
  double spec_error = 0.0;                // total error at that linearisation point (priors included)
  DevBuf packed_save;                     // linearize-at-candidate: the candidate's (reduced) system is formed here; an accepted
                                          // candidate swaps it with `packed` (which always is the current estimate's system)
  TermSide terms;                         // keypoint and pose-graph terms: as added, this rank's layout, device tables, results
  PriorSide priors;                       // marginal-prior terms: as added, this rank's layout, device arrays (window_prior.hip)
  uint64_t results_epoch = 0;             // == vars_epoch: the per-edge and per-term results are the linearisation at the current variables
  FactorCache fc;                         // f2: the per-Values factor cache (sage_window_prepass): window_state.h
  uint64_t dense_serial = 0;              // counts the linearizes that have written dense[].AtA (FactorSlot::live_serial)
  DoglegSide dogleg;                      // the dogleg step's tables, vectors and pinned dots (window_dogleg.hip)
  RelinSide relin;                        // partial relinearization: mode, snapshot, depth stamps, sub work lists (window_relin.hip)
  CovarianceSide cov;                     // marginal covariances of the last solve, opt-in (window_covariance.hip)
  TsdfSide tsdf;                          // scratch of sage_window_fuse_tsdf and sage_window_depth_range (window_tsdf.hip)
  WindowProfiler prof;            // optional kernel timing (window_profile.hip)

  // do the assembly and the error pass mirror their totals into pinned memory themselves?  Single-rank windows WITHOUT an
  // all-reduce hook only (a reduced total is mirrored after the sum: mirror_totals_kernel; a one-rank RCCL communicator or
  // sage_window_set_allreduce leaves the mirror to that kernel too).  The ONE condition writers and readers share
  bool kernels_mirror_totals() const { return world == 1 && !dist.allreduce && mirror.h; }
};


// shared between the window translation units
template <class T>
static int upload(DevBuf &b, const std::vector<T> &v, hipStream_t s)
{
  int rc = b.reserve(std::max<size_t>(v.size(), 1) * sizeof(T));
  if (rc)
    return rc;
  if (!v.empty())
    SAGE_HIP(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  return 0;
}
// window.hip
int window_upload_vars(SageWindow *w, int set);
int window_local_edge(const SageWindow *w, int global_edge); // local index of DENSE directed edge 2 * link + dir, or -1
bool window_owns_edge(const SageWindow *w, int global_edge);  // is directed edge 2 * link + dir this rank's?
bool window_has_holds(const SageWindow *w);
std::vector<int32_t> window_link_pairs(const SageWindow *w);  // [nlinks][2]: the links as the host solvers take them
// window_build.hip: what the stages of sage_window_finalize hand to one another; on the host for the length of the call
struct FinalizeState
{
  bool domain_solve = false;               // plan::uses_domain_solve, asked once: ownership granularity and the shard plan
  std::vector<char> needed;                // [K]: keyframes this rank's links touch
  std::vector<size_t> f0s_off;             // [K + 1]: floats of pre-sampled source features before keyframe k
  std::vector<size_t> px_off;              // [n_edges + 1]: source pixels before local edge e (rows of geo_px)
  std::vector<int> Nedge;                  // samples (slots) per local directed edge
  std::vector<std::vector<AdjEntry>> adjv; // [K]: the keyframe's (edge, role) incidences, the terms' included
  std::vector<LinkEdges> le;               // per link: its local dense edges
  std::vector<char> link_terms;            // per link: it carries a local term
  double residuals = 0, bytes = 0;         // per linearize
};
// window_terms.hip
int finalize_terms(SageWindow *w, FinalizeState &fs);  // stage 7 of sage_window_finalize
int window_launch_terms(SageWindow *w, int set, bool jac); // the keypoint kernel, then the graph kernel, over this rank's terms
// window_prior.hip
int finalize_priors(SageWindow *w);                          // stage 7b of sage_window_finalize
int window_launch_prior_eval(SageWindow *w, int set, bool jac); // prior_eval_kernel over this rank's prior terms
int window_launch_prior_add(SageWindow *w, double *packed, double *tail_mirror); // prior_add_kernel behind the assembly of `packed`
const double *window_prior_partials(const SageWindow *w, bool jac, int *n_terms); // the pass's tile partials (null: no local term)
// window_eval.hip
// stale_only: the stale-mode linearize of sage_window_linearize (set 0 into `packed`, unmerged); every other call evaluates
// every edge and, in SAGE_RELIN_STALE, leaves every edge stale
int window_linearize_set(SageWindow *w, int set, double *dst = nullptr, bool local_blocks = false, bool merge = false,
                         bool stale_only = false);
int window_error_pass(SageWindow *w, int which, bool speculate_gradients);
// window_reduce.hip
int window_collective(SageWindow *w, double *buf, size_t n);                 // the hook's sum in place, nothing else
int window_allreduce(SageWindow *w, double *buf, size_t n, int iterate);     // ... + the emulated peers' share at `iterate`
int window_allreduce_into(SageWindow *w, const double *send, double *recv, size_t n, int iterate); // the same out of place
int window_mirror_totals(SageWindow *w, bool with_err, const double *system = nullptr); // enqueue totals + tickets -> mirror
bool window_wait_error_totals(SageWindow *w);   // spin on the last error pass's tickets; false: none to come / timed out
bool window_wait_reduced_totals(SageWindow *w); // ... on the last window_mirror_totals'
int window_wait_mirror(SageWindow *w, bool *not_psd); // the reduced totals and the candidate, a synchronise only on a time-out
double mirrored_error(const SageWindow *w, int at, int set); // mirror.h[at] + mirror.h[at + 1] + the priors at `set`
int window_total_error(SageWindow *w, int from_linearize, double *err, bool stream_idle);
int window_copy_floats(SageWindow *w, const float *src, float *dst, int n); // one-launch device copy on the window's stream
void window_add_to_double(SageWindow *w, double *p, double v);              // p[0] += v on the window's stream
// window_solve.hip
double window_prior_error(const SageWindow *w, int set, bool owned_only = false);
SolvePriors window_solve_priors(const SageWindow *w); // (damped_system.h) the priors as the scatter kernel takes them
int window_sync_candidate(SageWindow *w, bool stream_idle = false);
int window_schur_solve(SageWindow *w, double damp, double *lin_error);
// window_relin.hip
// what a stale-mode linearize launches: per dense side (kPhoto, kGeo) the stale edges, their work items and where the
// compacted plan lies on the device
struct RelinLaunch
{
  bool nothing = false;              // values and packed system are current: the call launches nothing at all
  int n_edges[2] = {0, 0}, n_items[2] = {0, 0};
  const WorkItem *work[2] = {nullptr, nullptr};
  const int32_t *first[2] = {nullptr, nullptr}; // LaunchCommon::edge_first of the side (the photometric side's: of its records, if it has them)
  const int32_t *list[2] = {nullptr, nullptr};  // the stale edges, ascending: one finalize workgroup each
  bool any() const { return n_edges[0] + n_edges[1] > 0; }
};
int relin_prepare(SageWindow *w, RelinLaunch &rl);  // the stale edges against the snapshot, their depth maps, the compacted plan
void relin_commit(SageWindow *w, const RelinLaunch &rl); // the launches are enqueued: the current variables become the snapshot
void relin_stamp_maps(SageWindow *w, int set, bool depth, bool grad); // a whole-window depth batch at `set` has been enqueued
void relin_count_all(SageWindow *w, bool dense, bool depth, bool grad); // SageEvalCounts of a linearize of every edge
// window_covariance.hip
int covariance_refusal(const SageWindow *w);  // why the window cannot have a covariance at all, or SAGE_OK
bool covariance_current(const SageWindow *w); // the stored Sigma belongs to the solver's last factor
DepthSigmaEntry window_sigma_entry(const SageWindow *w, int k, float *out); // keyframe k's row of a sigma launch, S from the stored Sigma
// window_profile.hip
void prof_attach(SageWindow *w, int which, LaunchCommon &lc); // profiling: an event pair for kernel `which` (LaunchCommon::ev_*)
void window_phase_mark(SageWindow *w, int which); // profiling: record phase mark `which` on the window's stream
