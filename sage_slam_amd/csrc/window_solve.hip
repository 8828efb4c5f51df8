// window_solve.hip -- from a system to a candidate: the prior terms, the damped solve (device solver, or the host block solve
// of windows with duplicate links), the sharded windows' separator solve, taking up the candidate the device solver left in
// pinned memory, and what becomes of a candidate afterwards: accept, reset, the exchange of the owners' variables.
#include "damped_system.h"
#include "runtime_internal.h"

// prior error terms at a variable set (a9): code prior w*||c||^2/CS per keyframe (code_factor.cpp:99-104, zero
// prior code), scale prior on keyframe 0 w*(ln s0 - ln s)^2 (scale_factor.cpp:102-129), pose prior on kf 0.
// owned_only (sharded windows): the terms of the keyframes THIS rank owns (the other ranks' copies of their variables are
// stale here).  The owned sum takes keyframe 0's scale / pose terms right behind its code term, the full sum behind every
// keyframe's code term: each keeps its order, so neither total moves in the last bit
double window_prior_error(const SageWindow *w, int set, bool owned_only)
{
  const SageWindowConfig &c = w->cfg;
  double e = 0;
  auto keyframe0_terms = [&] {
    if (c.scale_prior_weight > 0)
    {
      const double d = std::log((double)w->hv.scale_init[0]) - std::log((double)w->hv.scale[set][0]);
      e += c.scale_prior_weight * d * d;
    }
    if (c.pose_prior_weight > 0)
    {
      double loc[6];
      sage::pose_local(&w->hv.pose[set][0], &w->hv.pose_init[0], loc);
      for (int i = 0; i < 6; ++i)
        e += c.pose_prior_weight * loc[i] * loc[i];
    }
  };
  for (int k = 0; k < w->K; ++k)
  {
    if (owned_only && sage_shard_keyframe_owner(w->dist.shard, k) != w->rank)
      continue;
    double s = 0;
    for (int i = 0; i < c.CS; ++i)
      s += (double)w->hv.code[set][(size_t)k * c.CS + i] * w->hv.code[set][(size_t)k * c.CS + i];
    e += c.code_prior_weight * s / c.CS;
    if (owned_only && k == 0)
      keyframe0_terms();
  }
  if (!owned_only)
    keyframe0_terms();
  return e;
}

sage::SolvePriors window_solve_priors(const SageWindow *w)
{
  const SageWindowConfig &c = w->cfg;
  sage::SolvePriors pri{};
  pri.code_w = c.code_prior_weight; pri.scale_w = c.scale_prior_weight; pri.pose_w = c.pose_prior_weight;
  pri.scale_init0 = w->hv.scale_init[0];
  std::copy_n(&w->hv.pose_init[0], 12, pri.pose_init0);
  return pri;
}

// diagonal priors (a9) at the current variables, for the host solves: what the scatter kernel adds on the device
static void window_priors(const SageWindow *w, std::vector<double> &dadd, std::vector<double> &gadd)
{
  const int K = w->K, B = w->B, CS = w->cfg.CS;
  const sage::SolvePriors pri = window_solve_priors(w);
  dadd.assign((size_t)K * B, 0.0);
  gadd.assign((size_t)K * B, 0.0);
  for (int k = 0; k < K; ++k)
    for (int r = 0; r < B; ++r)
      sage::prior_row(pri, k, r, CS, &w->hv.pose[0][(size_t)k * 12], w->hv.scale[0][k], &w->hv.code[0][(size_t)k * CS],
                      dadd[(size_t)k * B + r], gadd[(size_t)k * B + r], w->hold.empty() ? 0 : w->hold[k]);
}

// candidate = retract(current, delta).  local_only (sharded windows): only the keyframes this rank touches, the others
// keep their (stale) current values.  Held entries are copied bit for bit, as solve_retract_kernel does (se3_exp of a zero
// delta is not the identity in fp32, x + -0.0f may flip a sign bit)
static void window_retract_candidate(SageWindow *w, bool local_only)
{
  const int K = w->K, B = w->B, CS = w->cfg.CS;
  if (local_only)
    w->hv.copy_set(1, 0);
  for (int k = 0; k < K; ++k)
  {
    if (local_only && !sage_shard_keyframe_is_local(w->dist.shard, k))
      continue;
    const int hold = w->hold.empty() ? 0 : w->hold[k];
    float d6[6];
    for (int i = 0; i < 6; ++i)
      d6[i] = (float)w->delta[(size_t)k * B + i];
    if (hold & sage::kHoldPose)
      std::copy_n(&w->hv.pose[0][(size_t)k * 12], 12, &w->hv.pose[1][(size_t)k * 12]);
    else
      sage_pose_retract(&w->hv.pose[0][(size_t)k * 12], d6, &w->hv.pose[1][(size_t)k * 12]);
    for (int i = 0; i < CS; ++i)
      w->hv.code[1][(size_t)k * CS + i] =
          (hold & sage::kHoldCode) ? w->hv.code[0][(size_t)k * CS + i]
                                   : w->hv.code[0][(size_t)k * CS + i] + (float)w->delta[(size_t)k * B + 6 + i];
    w->hv.scale[1][k] = (hold & sage::kHoldScale) ? w->hv.scale[0][k] : w->hv.scale[0][k] + (float)w->delta[(size_t)k * B + 6 + CS];
  }
}

// After a device solve the candidate variables / delta live in the solver's pinned buffers until the stream has
// drained: refresh the host mirrors (set 1) here.  Returns SAGE_E_NOT_PSD when the factorisation hit a non-positive
// pivot (the candidate is then meaningless).
int window_sync_candidate(SageWindow *w, bool stream_idle)
{
  if (!w->cand_pending)
    return SAGE_OK;
  if (!stream_idle)
    SAGE_HIP(hipStreamSynchronize(w->stream));
  w->cand_pending = false;
  const DeviceSolver *S = w->solver;
  if (solver_host_status(S) != 0)
    return SAGE_E_NOT_PSD;
  const float *v = solver_host_vars(S);
  for (int k = 0; k < w->K; ++k)
    w->hv.unpack(1, k, w->cfg.CS, v + (size_t)k * w->VS);
  std::memcpy(w->delta.data(), solver_host_delta(S), w->delta.size() * sizeof(double));
  return SAGE_OK;
}

extern "C" int sage_window_solve(SageWindow *w, double damp, double *step_norm)
{
  if (!w || !w->finalized || !w->have_lin)
    return SAGE_E_STATE;
  const SageWindowConfig &c = w->cfg;
  const int K = w->K, B = w->B, CS = c.CS;
  if (w->solver)
  {
    // device path: nothing leaves HBM but the candidate's host mirror (pinned, async); no synchronisation here
    // unless the caller asks for the step norm
    int rc = window_sync_candidate(w); // an unconsumed earlier candidate (a re-solve with another damping)
    if (rc && rc != SAGE_E_NOT_PSD)
      return rc;
    if (w->dpt_set == 1)
      w->dpt_set = -1; // the solve rewrites the candidate set
    w->dogleg.solved0 = w->dogleg.products = false;
    rc = solver_run(w->solver, w->stream, w->packed.as<double>(), w->vars[0].as<float>(), w->vars[1].as<float>(), CS,
                    damp, window_solve_priors(w));
    if (rc)
      return rc;
    w->dogleg.solved0 = damp == 0.0; // (the Gauss-Newton point: what sage_window_dogleg_products starts from)
    window_phase_mark(w, 3);
    w->cand_pending = true;
    if (step_norm)
    {
      if ((rc = window_sync_candidate(w)))
        return rc;
      *step_norm = std::sqrt(solver_host_step_norm2(w->solver));
    }
    return SAGE_OK;
  }
  const size_t np = sage_window_packed_count(w);
  static const bool dbg = sage::env_flag("SAGE_DEBUG_TIMING");
  auto tnow = [] { return std::chrono::steady_clock::now(); };
  auto t_a = tnow();
  SAGE_HIP(hipStreamSynchronize(w->stream));
  auto t_b = tnow();
  SAGE_HIP(hipMemcpyAsync(w->host_packed.data(), w->packed.p, np * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  auto t_c = tnow();
  // no device solver: the window has duplicate links (solver_create refused them), the host block solve sums them
  std::vector<double> dadd, gadd;
  window_priors(w, dadd, gadd);
  const std::vector<int32_t> lk = window_link_pairs(w);
  const bool holds = window_has_holds(w);
  if (holds) // the held rule on the host copy (damped_system.h); `packed` itself is untouched
    sage::hold_packed(w->host_packed.data(), dadd.data(), gadd.data(), K, (int)w->links.size(), lk.data(), B, CS, w->hold.data());
  int rcs;
  if (w->rows.compact())
  {
    // every keyframe holds a whole group: the system of the kept rows only (damped_system.h: solver rows), solved at Bs;
    // the delta keeps its [K][B] layout, zeros on the dropped rows
    const int Bs = w->rows.Bs, nl = (int)w->links.size();
    std::vector<double> ps((size_t)(K + nl) * Bs * Bs + (size_t)K * Bs);
    std::vector<double> ds((size_t)K * Bs), gs((size_t)K * Bs), xs((size_t)K * Bs);
    sage::compact_packed(w->host_packed.data(), dadd.data(), gadd.data(), K, nl, B, Bs, w->rows.to_block.data(), ps.data(),
                         ds.data(), gs.data());
    if ((rcs = sage_block_solve(ps.data(), K, nl, lk.data(), Bs, damp, ds.data(), gs.data(), xs.data())))
      return rcs;
    std::fill(w->delta.begin(), w->delta.end(), 0.0);
    for (int k = 0; k < K; ++k)
      for (int s = 0; s < Bs; ++s)
        w->delta[(size_t)k * B + w->rows.to_block[s]] = xs[(size_t)k * Bs + s];
  }
  else if ((rcs = sage_block_solve(w->host_packed.data(), K, (int)w->links.size(), lk.data(), B, damp, dadd.data(),
                                   gadd.data(), w->delta.data()))) // (writes delta only on success)
    return rcs;
  if (holds) // exactly zero, whatever sign the substitution left
    for (int k = 0; k < K; ++k)
      for (int r = 0; r < B; ++r)
        if (sage::row_held(w->hold[k], r, CS))
          w->delta[(size_t)k * B + r] = 0.0;
  auto t_d = tnow();
  double nrm = 0;
  for (double v : w->delta)
    nrm += v * v;
  if (step_norm)
    *step_norm = std::sqrt(nrm);
  window_retract_candidate(w, false);
  const int rcu = window_upload_vars(w, 1);
  if (dbg)
  {
    auto t_e = tnow();
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[sage solve] wait-kernels %.3f d2h %.3f block_solve %.3f retract+h2d %.3f ms\n", ms(t_a, t_b),
            ms(t_b, t_c), ms(t_c, t_d), ms(t_d, t_e));
  }
  return rcu;
}

// local elimination -> all-reduce of the separator system -> separator solve + back substitution of this rank's
// keyframes -> candidate variables of those keyframes.  *lin_error (optional) receives the total error at the
// linearisation point (edge totals ride in the payload tail, prior terms are contributed by their owners).
// Returns SAGE_E_NOT_PSD consistently on every rank (a rank whose local elimination fails poisons the payload).
int window_schur_solve(SageWindow *w, double damp, double *lin_error)
{
  const int K = w->K, B = w->B;
  const size_t np = sage_window_packed_count(w), ns = w->dist.h_sep.size();
  SAGE_HIP(hipMemcpyAsync(w->host_packed.data(), w->packed.p, np * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  std::vector<double> dadd, gadd;
  window_priors(w, dadd, gadd);
  int rc = sage_shard_eliminate(w->dist.shard, w->host_packed.data(), damp, dadd.data(), gadd.data(), w->dist.h_sep.data());
  if (rc && rc != SAGE_E_NOT_PSD)
    return rc;
  if (rc == SAGE_E_NOT_PSD)
  {
    // a failed local elimination is flagged in the spare tail slot [ns-3] (a positive count after the sum: every rank
    // sees it); the separator blocks of this rank are void, the error totals at the linearisation point (tail[0..4],
    // written by sage_shard_eliminate before it factorises) stay finite so that st->error is valid on every rank
    std::fill(w->dist.h_sep.begin(), w->dist.h_sep.end() - 8, 0.0);
    w->dist.h_sep[ns - 3] = 1.0;
  }
  w->dist.h_sep[ns - 4] = window_prior_error(w, 0, true);
  SAGE_HIP(hipMemcpyAsync(w->dist.sepbuf.p, w->dist.h_sep.data(), ns * sizeof(double), hipMemcpyHostToDevice, w->stream));
  if ((rc = window_collective(w, w->dist.sepbuf.as<double>(), ns))) // (raw: the Schur sequence has no peer emulation)
    return rc;
  SAGE_HIP(hipMemcpyAsync(w->dist.h_sep.data(), w->dist.sepbuf.p, ns * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  if (lin_error)
    *lin_error = w->dist.h_sep[ns - 8] + w->dist.h_sep[ns - 7] + w->dist.h_sep[ns - 4];
  if (w->dist.h_sep[ns - 3] > 0.0 || std::isnan(w->dist.h_sep[0]))
    return SAGE_E_NOT_PSD;
  w->delta.assign((size_t)K * B, 0.0);
  rc = sage_shard_solve(w->dist.shard, w->dist.h_sep.data(), w->delta.data());
  if (rc)
    return rc; // SAGE_E_NOT_PSD of the separator system: identical on every rank
  window_retract_candidate(w, true);
  w->cand_pending = false;
  return window_upload_vars(w, 1);
}

extern "C" int sage_window_accept(SageWindow *w)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  int rcs = window_sync_candidate(w);
  if (rcs)
    return rcs;
  w->hv.copy_set(0, 1);
  w->dogleg.solved0 = w->dogleg.products = false; // (the dogleg vectors belong to the estimate that is replaced here)
  ++w->vars_epoch;
  ++w->dist.emu_cur;
  w->dpt_set = w->dpt_set == 1 ? 0 : -1; // depth maps evaluated at the candidate now belong to the current set
  return window_copy_floats(w, w->vars[1].as<float>(), w->vars[0].as<float>(), w->K * w->VS);
}

extern "C" int sage_window_reset(SageWindow *w)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  (void)window_sync_candidate(w);
  for (int s = 0; s < 2; ++s)
  {
    w->hv.pose[s] = w->hv.pose_init;
    w->hv.code[s] = w->hv.code_added;
    w->hv.scale[s] = w->hv.scale_init;
  }
  int rc;
  if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
    return rc;
  w->have_lin = false;
  w->dist.emu_cur = 0;
  w->relin.drop();
  return SAGE_OK;
}

// after a Schur-mode run every rank holds current variables only for the keyframes it touches: sum the owners' copies
extern "C" int sage_window_sync_variables(SageWindow *w)
{
  if (!w || !w->finalized)
    return SAGE_E_STATE;
  if (!w->dist.shard)
    return SAGE_OK; // every rank solves the whole system: nothing to exchange
  if (!w->dist.allreduce)
    return SAGE_E_STATE;
  const int K = w->K, CS = w->cfg.CS, VS = 13 + CS;
  std::vector<double> buf((size_t)K * VS, 0.0);
  for (int k = 0; k < K; ++k)
    if (sage_shard_keyframe_owner(w->dist.shard, k) == w->rank)
      w->hv.pack(0, k, CS, &buf[(size_t)k * VS]);
  int rc;
  {
    DevBuf d; // the collective's device buffer: gone with this block, on every way out of it
    if ((rc = d.reserve(buf.size() * sizeof(double))))
      return rc;
    SAGE_HIP(hipMemcpyAsync(d.p, buf.data(), buf.size() * sizeof(double), hipMemcpyHostToDevice, w->stream));
    if ((rc = window_collective(w, d.as<double>(), buf.size()))) // (raw: the Schur sequence has no peer emulation)
      return rc;
    SAGE_HIP(hipMemcpyAsync(buf.data(), d.p, buf.size() * sizeof(double), hipMemcpyDeviceToHost, w->stream));
    SAGE_HIP(hipStreamSynchronize(w->stream));
  }
  for (int s = 0; s < 2; ++s)
    for (int k = 0; k < K; ++k)
      w->hv.unpack(s, k, CS, &buf[(size_t)k * VS]);
  if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
    return rc;
  return SAGE_OK;
}

extern "C" int sage_window_get_delta(const SageWindow *w, double *delta)
{
  if (!w || !delta)
    return SAGE_E_INVALID;
  int rcs = window_sync_candidate(const_cast<SageWindow *>(w));
  if (rcs)
    return rcs;
  std::memcpy(delta, w->delta.data(), w->delta.size() * sizeof(double));
  return SAGE_OK;
}
