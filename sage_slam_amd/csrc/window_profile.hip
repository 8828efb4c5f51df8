// window_profile.hip -- optional kernel timing of a window (HIP events on its stream): a pool of recycled events, an event
// pair per profiled launch (prof_attach), the phase marks of an LM iteration (window_phase_mark) and the three entry points
// that switch it on and drain it.  Touches nothing else of the window but its stream.
#include "runtime_internal.h"

WindowProfiler::~WindowProfiler()
{
  for (auto &pm : phase_pending)
    for (auto &m : pm.ev)
      (void)hipEventDestroy(m.second);
  for (auto &m : phase_cur.ev)
    (void)hipEventDestroy(m.second);
  for (auto &pend : pending)
    for (auto &pr : pend)
    {
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  for (hipEvent_t e : ev_free)
    (void)hipEventDestroy(e);
}

static bool ev_get(WindowProfiler &pf, hipEvent_t *e)
{
  if (!pf.ev_free.empty())
  {
    *e = pf.ev_free.back();
    pf.ev_free.pop_back();
    return true;
  }
  return hipEventCreate(e) == hipSuccess;
}
static void ev_put(WindowProfiler &pf, hipEvent_t e)
{
  if (e)
    pf.ev_free.push_back(e);
}

void prof_attach(SageWindow *w, int which, LaunchCommon &lc)
{
  WindowProfiler &pf = w->prof;
  if (!pf.profiling || (pf.prof_level == 2 && which != 0))
    return;
  hipEvent_t a, b;
  if (!ev_get(pf, &a))
    return;
  if (!ev_get(pf, &b))
  {
    ev_put(pf, a);
    return;
  }
  lc.ev_start = a;
  lc.ev_stop = b;
  pf.pending[which].emplace_back(a, b);
}

void window_phase_mark(SageWindow *w, int which)
{
  WindowProfiler &pf = w->prof;
  if (!pf.profiling || pf.prof_level == 2)
    return;
  if (which == 0) // a new iteration: the previous one's marks are complete
  {
    if (pf.phase_cur.ev.size() >= 2)
    {
      if (pf.phase_pending.size() >= 1024) // nobody collects them: keep the newest
      {
        for (auto &m : pf.phase_pending.front().ev)
          ev_put(pf, m.second);
        pf.phase_pending.erase(pf.phase_pending.begin());
      }
      pf.phase_pending.push_back(std::move(pf.phase_cur));
    }
    else
      for (auto &m : pf.phase_cur.ev)
        ev_put(pf, m.second);
    pf.phase_cur = WindowProfiler::PhaseMarks{};
  }
  else if (pf.phase_cur.ev.empty())
    return; // (a mark outside an iteration: sage_window_solve / _error called on their own)
  hipEvent_t e;
  if (pf.phase_cur.ev.size() >= 64 || !ev_get(pf, &e))
    return;
  (void)hipEventRecord(e, w->stream);
  pf.phase_cur.ev.emplace_back(which, e);
}

extern "C" int sage_window_get_phase_time(SageWindow *w, double *ms4, int *iterations)
{
  if (!w || !ms4)
    return SAGE_E_INVALID;
  WindowProfiler &pf = w->prof;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  window_phase_mark(w, 0); // flush the iteration in progress
  for (auto &m : pf.phase_cur.ev) // (the mark the flush just recorded opens nothing)
    ev_put(pf, m.second);
  pf.phase_cur = WindowProfiler::PhaseMarks{};
  for (auto &pm : pf.phase_pending)
  {
    // the time between two consecutive marks belongs to the phase the later one closes (1 linearize, 2 all-reduce,
    // 3 solve, 4 error pass); every evaluation of an iteration counts
    double d4[4] = {0, 0, 0, 0};
    bool ok = true;
    for (size_t i = 1; i < pm.ev.size() && ok; ++i)
    {
      float d = 0.f;
      ok = hipEventElapsedTime(&d, pm.ev[i - 1].second, pm.ev[i].second) == hipSuccess;
      const int ph = pm.ev[i].first;
      if (ok && ph >= 1 && ph <= 4)
        d4[ph - 1] += d;
    }
    if (ok)
    {
      for (int i = 0; i < 4; ++i)
        pf.phase_ms[i] += d4[i];
      pf.phase_n += 1;
    }
    for (auto &m : pm.ev)
      ev_put(pf, m.second);
  }
  pf.phase_pending.clear();
  for (int i = 0; i < 4; ++i)
  {
    ms4[i] = pf.phase_ms[i];
    pf.phase_ms[i] = 0;
  }
  if (iterations)
    *iterations = pf.phase_n;
  pf.phase_n = 0;
  return SAGE_OK;
}

extern "C" int sage_window_set_profiling(SageWindow *w, int on)
{
  if (!w)
    return SAGE_E_INVALID;
  WindowProfiler &pf = w->prof;
  pf.profiling = on != 0;
  pf.prof_level = on;
  // a stock of events up front: creating them inside the region being profiled costs API time there
  while (pf.profiling && pf.ev_free.size() < 512)
  {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess)
      break;
    pf.ev_free.push_back(e);
  }
  return SAGE_OK;
}

extern "C" int sage_window_get_kernel_time(SageWindow *w, int which, double *total_ms, int *launches)
{
  if (!w || which < 0 || which > 9)
    return SAGE_E_INVALID;
  WindowProfiler &pf = w->prof;
  SAGE_HIP(hipStreamSynchronize(w->stream));
  for (auto &pr : pf.pending[which])
  {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess)
    {
      pf.prof_ms[which] += ms;
      pf.prof_n[which] += 1;
    }
    ev_put(pf, pr.first);
    ev_put(pf, pr.second);
  }
  pf.pending[which].clear();
  if (total_ms)
    *total_ms = pf.prof_ms[which];
  if (launches)
    *launches = pf.prof_n[which];
  pf.prof_ms[which] = 0;
  pf.prof_n[which] = 0;
  return SAGE_OK;
}
