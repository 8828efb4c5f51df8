// window_lm.hip -- the LM iteration on a finalized window: one policy around the steps of three sequences (classic, schur,
// at_candidate), each written as what it enqueues and then what it waits for; the n-iteration loops of the C ABI.
#include "runtime_internal.h"

// The LM iteration (sage_window_lm_step): one policy -- accept test, give-up test, damping schedule -- around the steps
// of one of three sequences, which take the same decisions and walk the same iterates.  classic: linearize (+ all-reduce
// of `packed`); per evaluation a damped solve and an error pass (+ all-reduce of its 4 totals).  schur (sharded windows
// with a shard plan): linearize; per evaluation a local elimination, an all-reduce of the separator system, the separator
// solve, an error pass and an all-reduce of its 4 totals.  at_candidate: per evaluation a damped solve and a linearize at the
// candidate into packed_save (its finalize kernels deliver the error); accepted: the two buffers swap -- the candidate's
// system IS the next iteration's, nothing is re-evaluated or copied; rejected: `packed` never left.
enum class LmSeq { classic, schur, at_candidate };

// (rank-independent decision: the window's link count, not this rank's share of it -- a rank without links must issue
//  the same collectives as the others).  linearize_at_candidate 0 = automatic: the sequence with one collective and no
//  separate error pass per iteration whenever the window is reduced over ranks (the shard's kernels are short there, the
//  second collective and its host round trip are not), the classic sequence on a single rank
static LmSeq lm_sequence_for(const SageWindow *w, const SageLmConfig *cfg)
{
  const bool sharded = w->dist.allreduce != nullptr; // (a hook on a single-rank window is honoured too)
  if (sharded && w->dist.shard)
    return LmSeq::schur;
  const bool at_candidate = cfg->linearize_at_candidate > 0 || (cfg->linearize_at_candidate == 0 && sharded);
  return at_candidate && !w->links.empty() ? LmSeq::at_candidate : LmSeq::classic;
}

// what one evaluation leaves for a later step of the same iteration
struct LmEval
{
  double cur_tot[4];  // at_candidate: the mirrored totals of the current estimate, put back by a rejection
  bool have_cur_tot;  // (a synchronous non-positive pivot of the solve leaves the mirror alone: nothing to put back)
};

// at_candidate: the (reduced) system at variable set `set` into dst, its totals into the pinned mirror with their tickets
// -- the host never blocks in a stream synchronise on the iteration's critical path.  A reduced window assembles only the
// blocks its own edges touch (into packed_loc) and sums out of place into dst; the emulated peers' share of iterate `it`
// is added behind the sum.  The caller books what dst holds now.
static int window_form_system(SageWindow *w, int set, double *dst, int it)
{
  int rc;
  if (!w->dist.allreduce)
    return (rc = window_linearize_set(w, set, dst, false, true)) ? rc : window_mirror_totals(w, false, dst);
  if ((rc = window_linearize_set(w, set, w->dist.packed_loc.as<double>(), true, true)) ||
      (rc = window_allreduce_into(w, w->dist.packed_loc.as<double>(), dst, sage_window_packed_count(w), it)))
    return rc;
  window_phase_mark(w, 2);
  return window_mirror_totals(w, false, dst);
}

// the system at the current estimate, before the first evaluation (at_candidate: and its error, st->error)
static int lm_prepare(LmSeq seq, SageWindow *w, SageLmState *st)
{
  int rc;
  const bool sharded = w->dist.allreduce != nullptr;
  const size_t np = sage_window_packed_count(w);
  if (seq != LmSeq::at_candidate)
  {
    if ((rc = window_linearize_set(w, 0, nullptr, false, true)) ||
        (seq == LmSeq::classic && sharded && (rc = window_allreduce(w, w->packed.as<double>(), np, w->dist.emu_cur))))
      return rc;
    window_phase_mark(w, 2);
    return SAGE_OK;
  }
  if ((rc = w->packed_save.reserve(np * sizeof(double))))
    return rc;
  if (sharded && !w->dist.packed_loc.p)
  {
    if ((rc = w->dist.packed_loc.reserve(np * sizeof(double))))
      return rc;
    SAGE_HIP(hipMemsetAsync(w->dist.packed_loc.p, 0, np * sizeof(double), w->stream)); // blocks of other ranks: zero for good
  }
  // the system at the current estimate is reused only if it is the GLOBAL one: sage_window_linearize / _prepass and the
  // classic sequence leave a system behind that is not booked as reduced (every rank sees the same flags: same call
  // sequence on all ranks)
  bool mirrored_now = false;
  if (!(w->have_lin && w->lin_epoch == w->vars_epoch && (!sharded || w->dist.packed_reduced)))
  {
    if ((rc = window_form_system(w, 0, w->packed.as<double>(), w->dist.emu_cur)))
      return rc;
    w->have_lin = true;
    w->lin_epoch = w->vars_epoch;
    w->dist.packed_reduced = true; // (summed over the ranks, or nothing to sum)
    w->spec_err_valid = false;
    mirrored_now = true;
  }
  if (!w->spec_err_valid)
  {
    // the totals at the current estimate: mirrored by the evaluation above -- or the system was left by
    // sage_window_linearize (unsharded: mirror its tail now)
    if (!mirrored_now && (rc = window_mirror_totals(w, false)))
      return rc;
    if (!window_wait_reduced_totals(w))
      SAGE_HIP(hipStreamSynchronize(w->stream));
    w->spec_error = mirrored_error(w, TotalsMirror::kTail, 0);
    w->spec_err_valid = true;
  }
  st->error = w->spec_error;
  return SAGE_OK;
}

// schur.  Enqueues (inside window_schur_solve, with its waits: the host factorises) the copy of the system, the separator
// payload and its all-reduce; then the error pass, the owned prior terms on top of its photometric total, the all-reduce of
// the 4 totals and their copy.  Waits for that copy.  A non-positive pivot, identical on every rank, ends it before the
// error pass
static int evaluate_schur(SageWindow *w, SageLmState *st, bool first)
{
  int rc;
  double lin_error = 0;
  if ((rc = window_schur_solve(w, st->damp, &lin_error)) && rc != SAGE_E_NOT_PSD)
    return rc;
  window_phase_mark(w, 3);
  if (first)
    st->error = lin_error;
  st->candidate_error = INFINITY;
  if (rc == SAGE_E_NOT_PSD)
    return SAGE_OK;
  if ((rc = sage_window_error(w, 1)))
    return rc;
  window_add_to_double(w, w->errbuf.as<double>(), window_prior_error(w, 1, true));
  if ((rc = window_collective(w, w->errbuf.as<double>(), 4))) // (raw: the Schur sequence has no peer emulation)
    return rc;
  double t4[4];
  SAGE_HIP(hipMemcpyAsync(t4, w->errbuf.p, sizeof(t4), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  st->candidate_error = t4[0] + t4[1];
  return SAGE_OK;
}

// at_candidate, behind the damped solve.  Enqueues the linearize at the candidate into packed_save, its sum over the ranks
// and the mirror of its totals; waits for the mirror's tickets and takes up the candidate.  The current estimate's
// mirrored totals are kept for a rejection
static int evaluate_at_candidate(SageWindow *w, SageLmState *st, LmEval &ev)
{
  int rc;
  std::memcpy(ev.cur_tot, w->mirror.h, sizeof(ev.cur_tot)); // (mirrored and seen at the end of the previous evaluation)
  ev.have_cur_tot = true;
  bool not_psd;
  if ((rc = window_form_system(w, 1, w->packed_save.as<double>(), w->dist.emu_cur + 1)) ||
      (rc = window_wait_mirror(w, &not_psd)))
    return rc;
  st->candidate_error = not_psd ? INFINITY : mirrored_error(w, TotalsMirror::kTail, 1);
  return SAGE_OK;
}

// classic, behind the damped solve.  Enqueues the error pass at the candidate.  Single rank: waits for the pass's own
// tickets and reads both totals from the mirror.  Reduced: enqueues the all-reduce of the 4 totals and their mirror, waits
// for the mirror's tickets
static int evaluate_classic(SageWindow *w, SageLmState *st, bool first)
{
  int rc;
  const bool sharded = w->dist.allreduce != nullptr;
  if ((rc = window_error_pass(w, 1, !sharded)))
    return rc;
  if (!sharded)
  {
    // the error at the linearisation point (tail of the packed buffer) is read together with the candidate's
    const bool idle = window_wait_error_totals(w);
    if (first && (rc = window_total_error(w, 1, &st->error, idle)))
      return rc;
    if ((rc = window_total_error(w, 0, &st->candidate_error, idle)) == SAGE_E_NOT_PSD)
      st->candidate_error = INFINITY;
    return rc == SAGE_E_NOT_PSD ? SAGE_OK : rc;
  }
  bool not_psd;
  if ((rc = window_allreduce(w, w->errbuf.as<double>(), 4, w->dist.emu_cur + 1)) || (rc = window_mirror_totals(w, true)) ||
      (rc = window_wait_mirror(w, &not_psd)))
    return rc;
  if (first)
    st->error = mirrored_error(w, TotalsMirror::kTail, 0);
  st->candidate_error = not_psd ? INFINITY : mirrored_error(w, TotalsMirror::kError, 1);
  return SAGE_OK;
}

// one damped solve at st->damp and the candidate's error -> st->candidate_error (INFINITY for a non-positive pivot,
// reported by the solve at once or by window_sync_candidate: a rejected evaluation, not a hard error -- every rank factors
// the same reduced system, so all of them take that branch together and issue the same collectives).  first: classic and
// schur learn st->error here
static int lm_evaluate(LmSeq seq, SageWindow *w, SageLmState *st, bool first, LmEval &ev)
{
  if (seq == LmSeq::schur)
    return evaluate_schur(w, st, first); // (the solve is its own: the separator system's)
  // everything of one evaluation is enqueued before the host looks at a number
  const int rc = sage_window_solve(w, st->damp, nullptr);
  if (rc == SAGE_E_NOT_PSD) // (no error pass, no collective)
  {
    st->candidate_error = INFINITY;
    return first && seq == LmSeq::classic ? sage_window_total_error(w, 1, &st->error) : SAGE_OK;
  }
  if (rc)
    return rc;
  return seq == LmSeq::at_candidate ? evaluate_at_candidate(w, st, ev) : evaluate_classic(w, st, first);
}

// the candidate becomes the current estimate (at_candidate: and its system, formed in packed_save, the current system)
static int lm_accept(LmSeq seq, SageWindow *w, const SageLmState *st)
{
  const int rc = sage_window_accept(w);
  if (rc || seq != LmSeq::at_candidate)
    return rc;
  w->packed.swap(w->packed_save);
  w->lin_epoch = w->vars_epoch;
  w->results_epoch = w->vars_epoch; // (the last linearize was the accepted candidate's: its per-edge results are current too)
  w->dist.packed_reduced = true; // (summed over the ranks by window_form_system, or nothing to sum)
  w->spec_error = st->candidate_error;
  return SAGE_OK;
}

// the candidate is dropped (at_candidate: the mirror goes back to the current estimate's totals)
static void lm_reject(SageWindow *w, const LmEval &ev)
{
  if (ev.have_cur_tot)
    std::memcpy(w->mirror.h, ev.cur_tot, sizeof(ev.cur_tot));
}

extern "C" int sage_window_lm_step(SageWindow *w, SageLmState *st, const SageLmConfig *cfg)
{
  if (!w || !st || !cfg)
    return SAGE_E_INVALID;
  if (w->world > 1 && !w->dist.allreduce)
    return SAGE_E_STATE;
  const LmSeq seq = lm_sequence_for(w, cfg);
  auto clampd = [&](double d) { return std::min(std::max((double)cfg->min_damp, d), (double)cfg->max_damp); };
  if (st->iters == 0 && st->damp <= 0)
    st->damp = cfg->init_damp;
  window_phase_mark(w, 0);
  int rc = lm_prepare(seq, w, st);
  if (rc)
    return rc;
  st->accepted = 0;
  for (int evals = 1;; ++evals)
  {
    LmEval ev{};
    if ((rc = lm_evaluate(seq, w, st, evals == 1, ev)))
      return rc;
    if (st->candidate_error < st->error)
    {
      st->accepted = 1;
      if ((rc = lm_accept(seq, w, st)))
        return rc;
      st->damp = clampd(st->damp / cfg->damp_dec_factor);
      break;
    }
    lm_reject(w, ev);
    const bool give_up = st->damp >= cfg->max_damp || (cfg->max_inner_evals > 0 && evals >= cfg->max_inner_evals);
    st->damp = clampd(st->damp * cfg->damp_inc_factor);
    if (give_up)
      break;
  }
  st->iters += 1;
  return SAGE_OK;
}

// n LM iterations in one call (the loop a C++ caller writes around sage_window_lm_step; bench.py uses it so that no Python
// runs between the iterations it times).  trace (optional): n x {error, candidate_error, accepted, damp after the step}.
// Stops early on an error code; *done (optional) = iterations completed.
static int window_lm_run(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace, int *done,
                         double *step_seconds)
{
  if (!w || !st || !cfg || n < 0)
    return SAGE_E_INVALID;
  int i = 0, rc = SAGE_OK;
  auto t_prev = std::chrono::steady_clock::now();
  for (; i < n; ++i)
  {
    if ((rc = sage_window_lm_step(w, st, cfg)))
      break;
    if (trace)
    {
      trace[4 * i + 0] = st->error;
      trace[4 * i + 1] = st->candidate_error;
      trace[4 * i + 2] = (double)st->accepted;
      trace[4 * i + 3] = st->damp;
    }
    if (step_seconds)
    {
      const auto t = std::chrono::steady_clock::now();
      step_seconds[i] = std::chrono::duration<double>(t - t_prev).count();
      t_prev = t;
    }
  }
  if (done)
    *done = i;
  return rc;
}

extern "C" int sage_window_lm_run(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace, int *done)
{
  return window_lm_run(w, st, cfg, n, trace, done, nullptr);
}

// the same with the host wall time of every iteration (step_seconds[n]: from the return of the previous iteration -- the
// call's entry for the first -- to this one's; an iteration returns once its accept / reject decision is taken)
extern "C" int sage_window_lm_run_timed(SageWindow *w, SageLmState *st, const SageLmConfig *cfg, int n, double *trace,
                                        int *done, double *step_seconds)
{
  return window_lm_run(w, st, cfg, n, trace, done, step_seconds);
}
