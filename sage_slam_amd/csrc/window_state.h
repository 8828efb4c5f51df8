// window_state.h -- the parts SageWindow (runtime_internal.h) is made of, one struct per owner: the host variables, a dense
// factor type's device state, the terms, the factor cache, the totals mirror, the distributed state, the profiler.  Included from runtime_internal.h
// (after DevBuf); host code only.
#pragma once

namespace sage_rt
{

enum : int { kPhoto = 0, kGeo = 1 }; // dense factor types: AdjEntry::type, the `type` of the C ABI

// columns of a dense factor type's per-edge system
static inline size_t dense_dim(int type, int CS) { return type == kPhoto ? 13 + (size_t)CS : 14 + 2 * (size_t)CS; }

// ---- host variables: [set][kf]; set 0 = current, 1 = candidate ----
struct HostVars
{
  std::vector<float> pose[2], code[2], scale[2];
  std::vector<float> code_init, scale_init, pose_init;
  std::vector<float> code_added; // codes as added (code_init is the zero prior mean)
  void copy_set(int dst, int src) { pose[dst] = pose[src], code[dst] = code[src], scale[dst] = scale[src]; }

  // a keyframe's record of the [K][VS] device layout: pose 12, scale 1, code CS (T: float on the device, double as the
  // payload of sage_window_sync_variables)
  template <class T>
  void pack(int set, int k, int CS, T *rec) const
  {
    for (int i = 0; i < 12; ++i)
      rec[i] = pose[set][(size_t)k * 12 + i];
    rec[12] = scale[set][k];
    for (int i = 0; i < CS; ++i)
      rec[13 + i] = code[set][(size_t)k * CS + i];
  }
  template <class T>
  void unpack(int set, int k, int CS, const T *rec)
  {
    for (int i = 0; i < 12; ++i)
      pose[set][(size_t)k * 12 + i] = (float)rec[i];
    scale[set][k] = (float)rec[12];
    for (int i = 0; i < CS; ++i)
      code[set][(size_t)k * CS + i] = (float)rec[13 + i];
  }
};

// ---- one dense factor type (photometric / geometric) on the device ----
struct DenseSide
{
  DevBuf tab[2];              // edge table per variable set (PhotoEdge / GeoEdge)
  DevBuf work, first, tiles;  // work list: items, per edge its first item and its number of items
  DevBuf part;                // workgroup partials
  DevBuf AtA, Atb;            // per-edge results
  DevBuf stats;               // [2][n_res][2]: {error, inliers} of the last linearize, of the last error pass -- apart, as the
                              // terms' are: the linearization's statistics of an edge survive an error pass at other values
  DevBuf wide;                // ... before their fp32 rounding (EdgeOut::wide)
  int n_work = 0, tpb = 1;
  size_t n_res = 0;           // edges the result buffers have room for
  std::vector<int32_t> h_tiles; // host copy of `tiles` (the stale-mode linearize sizes its grids from it)
  EdgeOut out() const { return EdgeOut{AtA.as<float>(), Atb.as<float>(), stats.as<float>(), wide.as<double>()}; }
  float *error_stats() const { return stats.as<float>() + 2 * n_res; } // the error pass's half
  // room for the results of `ne` edges with D columns and for `records` partials of `partial_floats` floats
  int reserve_results(size_t ne, size_t D, size_t records, size_t partial_floats)
  {
    int rc;
    if ((rc = part.reserve(std::max<size_t>(1, records) * partial_floats * sizeof(float))) ||
        (rc = AtA.reserve(ne * D * D * sizeof(float))) || (rc = Atb.reserve(ne * D * sizeof(float))) ||
        (rc = stats.reserve(2 * ne * 2 * sizeof(float))) || (rc = wide.reserve(ne * (D * D + D) * sizeof(double))))
      return rc;
    n_res = ne;
    return 0;
  }
};

// ---- the window's keypoint and pose-graph terms: host copies as added, then (finalize) this rank's on the device ----
struct KeypointTermHost
{
  int32_t kind, edge, N, loss;
  float loss_param, weight;
  std::vector<int32_t> loc0, loc1;
  std::vector<float> homo0, second; // second: matched_2d [N,2] (reprojection) or matched_homo1 [N,3] (match geometry, loop-MG)
  std::vector<float> dpts0, dpts1;  // loop-MG: the unscaled depths [N]
};
struct TermSide
{
  std::vector<KeypointTermHost> kp_added; // sage_window_add_keypoint_term
  std::vector<SageGraphTerm> gt_added;    // sage_window_add_graph_term
  plan::TermLayout layout;                // which of them are this rank's and where each one lives
  DevBuf pool, kp_table, gt_table;        // the keypoint terms' arrays behind their table (KpTerm); the graph terms' (GraphTerm)
  DevBuf link_start, link;                // per link the terms on its two directions (AdjEntry::role = direction)
  DevBuf AtA[plan::kTermGroups], Atb[plan::kTermGroups]; // per group [count][D * D], [count][D]
  DevBuf stats;                           // [2][n_stats][2]: {error, inliers} of the last linearize, of the last error pass
  bool linearized = false;                // ... at least once: there is something to read
  uint64_t serial = 0;                    // counts the linearizes that have written AtA / Atb (sage_window_prepare_factors_device)
  int n_keypoint() const { return layout.n_keypoint(); } // local terms of the keypoint kernel, of the graph kernel, of both
  int n_graph() const { return layout.n_graph(); }
  int n_stats() const { return layout.n_stats(); }
  // mask of the keypoint kinds present among the local terms (the keypoint kernel's LDS size)
  unsigned keypoint_kinds() const
  {
    unsigned m = 0;
    for (int id : layout.kp_order)
      m |= 1u << kp_added[id].kind;
    return m;
  }
  // the results of the linearize (jac) or of the error pass: the same systems, each pass its half of `stats`
  TermResults results(bool jac) const
  {
    float *st = n_stats() ? stats.as<float>() + (jac ? 0 : (size_t)2 * n_stats()) : nullptr; // (all zero without terms)
    return TermResults{AtA[0].as<float>(), Atb[0].as<float>(), AtA[1].as<float>(), Atb[1].as<float>(), AtA[2].as<float>(),
                       Atb[2].as<float>(), st, layout.count[0], layout.count[1], layout.count[2]};
  }
  // room for every group's systems and for `stats`, zeroed on stream s
  int reserve_results(int CS, hipStream_t s)
  {
    const size_t bytes = (size_t)2 * n_stats() * 2 * sizeof(float);
    int rc = stats.reserve(bytes);
    for (int g = 0; g < plan::kTermGroups && !rc; ++g)
    {
      const size_t n = std::max(1, layout.count[g]), D = TermResults::dim(g, CS);
      if (!(rc = AtA[g].reserve(n * D * D * sizeof(float))))
        rc = Atb[g].reserve(n * D * sizeof(float));
    }
    return rc ? rc : (int)hipMemsetAsync(stats.p, 0, bytes, s);
  }
};

// ---- the window's marginal-prior terms (window_prior.hip): copies of the priors as added, then (finalize) this rank's on the
// device behind one table, the image of their Lambda blocks in the packed layout, the per-keyframe lists of their Atb rows ----
struct PriorSide
{
  struct Added
  {
    SageMarginalPrior prior;
    std::vector<int32_t> kf_map;
  };
  std::vector<Added> added;     // sage_window_add_prior_term
  marg::PriorLayout layout;     // (finalize) which are this rank's, where their blocks land
  std::vector<marg::PriorTermDev> h_table; // host copy of `table` (offsets for sage_window_get_prior_term, sage_window_marginalize)
  DevBuf table, lambda, eta, x0; // the local terms' rows and arrays
  DevBuf atb[2], part[2];       // per pass (0: linearize, 1: error pass): Atb [sum n]; per row tile {delta^T Lambda delta, eta^T delta}
  DevBuf image, image_blocks;   // [n_blocks][B * B] doubles and the packed block each belongs to
  DevBuf grad, grad_start;      // PriorGradRow entries keyframe-major; per gradient workgroup its first entry (+ the end)
  int n_tiles = 0, n_blocks = 0, n_grad_kf = 0;
  bool evaluated = false;       // a linearize has written atb[0] / part[0]
  int n_local() const { return (int)layout.local.size(); }
};

// ---- f2: the per-Values factor cache behind the gtsam adapter (sage_window_prepass, window_factors.hip): host copies of this
// rank's systems and the values (all K keyframes) they were evaluated at ----
struct FactorSlot // the entries of one layout: a dense factor type's local directed edges, or a term group's entries
{
  size_t D = 0;                      // columns of an entry's system
  std::vector<float> A, b;           // [n][D][D], [n][D]: AtA / Atb as they lie on the device
  std::vector<double> C;             // the projected (NearestPsd) matrices in A's layout, once prepared (a factor that owns
                                     // fewer than D columns: its own sub-matrix, in place)
  DevBuf psd_in, psd_out, psd_stats; // device preparation: the uploaded A (only when the device's own has moved on), the
                                     // projected matrices, the records
  const DevBuf *live = nullptr;          // the device AtA that A was pulled from ...
  const uint64_t *live_serial = nullptr; // ... the count of the linearizes that have written it ...
  uint64_t serial = 0;                   // ... and its value at the pull: equal -> `live` still is the cached linearisation
  size_t n() const { return D ? A.size() / (D * D) : 0; }
  const float *live_AtA() const { return live && serial == *live_serial ? live->as<float>() : nullptr; }
};
struct FactorCache
{
  enum : int { kSlots = 2 + plan::kTermGroups, kStatSets = 3 }; // slots kPhoto, kGeo, 2 + g: term group g
  bool lin = false, err = false;
  std::vector<float> pose, code, scale; // the key: [K][12], [K][CS], [K]
  FactorSlot slot[kSlots];
  // {error, inliers} of the pass the cache was pulled from: [kPhoto], [kGeo] per local directed edge, [2] per term (n_stats)
  std::vector<float> stats[kStatSets];
  int psd_mode = -1;                    // < 0: the projected matrices are not prepared for the cached linearisation
  // SAGE_RELIN_STALE: the dense slots' host rows are kept while they mirror the device's per-edge results (the values those
  // stand for: RelinSide's snapshot) -- the count of SageWindow::dense_serial at the last pull, once there was one
  bool rows_pulled = false;
  uint64_t rows_serial = 0;
  int psd_launches = 0;                 // sage_window_prepare_factors_device: what the last call launched ...
  SagePsdStats psd_worst{};             // ... and its worst record
};

// photometric linearize only: partial RECORDS per edge (`flush` sub-tiles each; the error pass counts work items)
struct PhotoRecordPlan
{
  DevBuf first, count;
  int flush = 0, n = 0;
  std::vector<int32_t> h_count; // host copy of `count`
};

// ---- partial relinearization (sage_window_set_relinearization, window_relin.hip).  The snapshot: the values every per-edge
// linearization on the device stands for -- after a stale-mode linearize each edge was either evaluated at them or read
// nothing that differs from them.  The stamps: depth maps are shared by the variable sets and rewritten by every error pass,
// so each keyframe's map carries the code and scale bits it was built from and whether its gradient was built from it ----
struct RelinSide
{
  int mode = 0;                          // SAGE_RELIN_*
  bool valid = false;                    // the snapshot holds; false: every edge is stale
  bool packed_current = false;           // `packed` was assembled from the results the snapshot stands for
  std::vector<float> pose, code, scale;  // the snapshot: [K][12], [K][CS], [K]
  std::vector<float> map_code, map_scale; // the stamps: [K][CS], [K] ...
  std::vector<uint8_t> map_ok, grad_ok;  // ... [K]: the map / its gradient is what the stamp says
  std::vector<DepthItem> depth_items;    // host copy of variable set 0's depth items, by keyframe ([K]; unused ones zero)
  DevBuf work_sub[2], first_sub[2];      // per dense side: the stale edges' work items in their order; per edge (full
                                         // length) the compacted first item, written at the stale edges' entries only
  DevBuf rec_first_sub;                  // the same for the photometric linearize's partial records
  DevBuf lists, depth_sub;               // what the host sends per call: stale edges and offsets; the depth items to rebuild
  PinnedBuf stage_lists, stage_depth;    // ... as the host writes them; stage_free: the copies out of them have been made
  hipEvent_t stage_free = nullptr;
  bool stage_busy = false;
  std::vector<int32_t> evaluated[2];     // local edges the last stale-mode linearize evaluated, ascending (a prepass pulls these rows)
  SageEvalCounts counts{};               // sage_window_last_evaluation
  void drop() { valid = packed_current = false; }
  RelinSide() = default;
  RelinSide(const RelinSide &) = delete;
  RelinSide &operator=(const RelinSide &) = delete;
  ~RelinSide()
  {
    if (stage_free)
      (void)hipEventDestroy(stage_free);
  }
};

// ---- pinned mirror of the totals, written by the kernels; the host spins on the tickets instead of synchronising ----
struct TotalsMirror
{
  // slot groups of h[kDoubles]: the linearize tail {err_photo, err_geo, n_photo, n_geo}, the error pass's totals (same
  // order), the tickets of error_totals_kernel, the tickets of mirror_totals_kernel
  enum : int { kTail = 0, kError = 4, kErrorTickets = 8, kMirrorTickets = 12, kDoubles = 16 };
  PinnedBuf mem;             // allocated and zeroed by finalize
  double *h = nullptr;       // = mem, once it is there
  uint64_t err_epoch = 0;    // ticket value of the last error pass
  uint64_t mirror_epoch = 0; // ticket value of the last mirror_totals_kernel
  // spin until the four tickets of `ticket_group` (kErrorTickets / kMirrorTickets) show `epoch`: what their kernel wrote before
  // them is in h then, and everything enqueued ahead of that kernel has landed.  Instead of a stream synchronise: a host
  // thread blocked there for more than a few dozen microseconds wakes up through an interrupt, 20-30 us after the kernel
  // has finished -- on the LM iteration's critical path.  false: timed out (the caller synchronises the stream)
  bool wait(int ticket_group, uint64_t epoch) const
  {
    const double *t = h + ticket_group;
    const double want = (double)epoch;
    auto ticket = [t](int i) {
      double v;
      __atomic_load(t + i, &v, __ATOMIC_ACQUIRE); // (a plain load on x86; the device is the writer)
      return v;
    };
    return spin_until([&] { return ticket(0) == want && ticket(1) == want && ticket(2) == want && ticket(3) == want; });
  }
};

// ---- the dogleg step (window_dogleg.hip): everything is allocated by the first call that needs it ----
struct DoglegSide
{
  DevBuf tables;          // int32: offsets [K + 1] | entries [K + 2 nlinks][2] (sage_dogleg_incidence) | links [nlinks][2]
  DevBuf part;            // the block kernel's partial products: [dogleg::partial_slots][2][B]
  DevBuf vec;             // g | Ag | n | An, [K * B] doubles each; n is fetched from the solve's pinned delta mirror
  DevBuf x;               // a trial point a g + b n in the solver's solution layout (SolverLayout): what the retraction reads
  PinnedBuf host;         // dogleg::HostRecord: the dots behind their ticket
  uint64_t epoch = 0;     // ticket value of the last products call
  bool ready = false;     // the buffers above are there
  bool solved0 = false;   // the candidate of the current system is the device solver's at damping 0 ...
  bool products = false;  // ... and g, Ag, n, An are that system's
  bool vectors = false;   // a products call has filled them (sage_window_get_dogleg_vectors reads the last call's)
};

// ---- the marginal covariances of the last solve (window_covariance.hip): Sigma's blocks on the host, in keyframe ids and the
// window's row order (pose 6, code CS, scale), zeros on held and dropped rows; everything is built by the first call ----
struct CovarianceSide
{
  cov::CovPlan plan;          // the closed pattern of the solver's elimination plan (once per window)
  bool planned = false;
  std::vector<double> work;   // Sigma on that pattern, in positions and padded solver rows: what the recursion writes
  std::vector<double> diag;   // [K][B * B]
  std::vector<double> link;   // [nlinks][B * B]: rows of the link's first keyframe, columns of its second
  bool valid = false;         // diag / link are Sigma of solve number `epoch` (SolverFactor::epoch) ...
  unsigned epoch = 0;
  double damp = 0.0;          // ... which was damped by this
  DepthSigmaStage stage;      // sage_window_depth_sigma's table and fp32 covariances
};

// ---- fusing the window's keyframes into a TSDF volume (window_tsdf.hip), opt-in: everything is built by the first call ----
struct TsdfSide
{
  DevBuf depth;      // [n][H * W]: the listed keyframes' depth maps at the current variables
  DevBuf sigma;      // [n][H * W]: the sigma maps of a SAGE_TSDF_STD_SIGMA fuse
  PinnedBuf range;   // sage_window_depth_range: the kernel's (min, max) [n][2]
};

// ---- sharded windows ----
struct WindowDist
{
  SageAllReduceFn allreduce = nullptr; // caller-provided sum all-reduce (see sage_ba.h)
  // optional out-of-place form of the hook (native RCCL: send != recv); without it: copy + in-place hook
  int (*allreduce2)(const double *send, double *recv, size_t n, void *user) = nullptr;
  void *allreduce_user = nullptr;
  void *rccl_hook = nullptr;           // sage_window_use_rccl: owned {comm, stream} record behind `allreduce`
  // domain-decomposed solve (shard_solve.cpp): the all-reduced payload is the separator system
  SageShardPlan *shard = nullptr;
  DevBuf sepbuf;                       // device copy of the separator buffer (what the collective sums)
  std::vector<double> h_sep;
  // development aid (sage_window_emulate_peers): after every all-reduce the contribution of the ranks that are not there
  // is added from a caller-provided table of packed systems (one per LM iterate since the last reset)
  const double *emu_rest = nullptr;
  int emu_n = 0, emu_cur = 0;          // emu_cur: index of the current iterate (reset -> 0, accept -> +1)
  DevBuf packed_loc;                   // reduced windows: this rank's un-reduced share (only the blocks its edges touch are
                                       // ever written, the rest stays zero), the send buffer of the out-of-place all-reduce
  DevBuf asm_blocks;                   // ids of those blocks (keyframes, links, tail) for the assembly of packed_loc
  int n_asm_blocks = 0;
  bool packed_reduced = false;         // `packed` has been summed over the ranks since it was last assembled
};

// ---- optional kernel timing (HIP events on the window's stream): window_profile.hip ----
struct WindowProfiler
{
  // phase marks of an LM iteration on the stream's timeline: 0 start of the iteration, 1 system assembled, 2 all-reduce of
  // the system enqueued / done, 3 candidate written (scatter + host factorisation + retract), 4 error pass done.  An
  // iteration is the list of marks in the order they were recorded (the classic sequence and the linearize-at-candidate
  // one order them differently, a rejected evaluation repeats some): the time between two consecutive marks is booked to
  // the phase the LATER mark closes
  struct PhaseMarks
  {
    std::vector<std::pair<int, hipEvent_t>> ev; // (mark, event) in the order they were recorded
  };
  std::vector<PhaseMarks> phase_pending;
  PhaseMarks phase_cur;
  double phase_ms[4] = {0, 0, 0, 0}; // linearize, all-reduce, solve, error pass
  int phase_n = 0;
  bool profiling = false;
  int prof_level = 0; // 1: all hot kernels + phase marks, 2: the photometric linearize only
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[10]; // (4 / 5: keypoint-term linearize / error launch, 6 / 7: graph-term,
                                                               //  8 / 9: prior_eval_kernel / prior_add_kernel)
  std::vector<hipEvent_t> ev_free; // recycled events (creating / destroying one per mark costs API time inside the region being profiled)
  double prof_ms[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int prof_n[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  WindowProfiler() = default;
  WindowProfiler(const WindowProfiler &) = delete;
  WindowProfiler &operator=(const WindowProfiler &) = delete;
  ~WindowProfiler(); // destroys every event it holds
};

} // namespace sage_rt
