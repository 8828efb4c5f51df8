// window.hip -- a finalized window as its other translation units and the caller see it: sizes and device buffers of the packed
// system, a keyframe's variables in and out, and the small helpers the units share.  Evaluating the factors is
// window_eval.hip, sums over ranks and the totals window_reduce.hip, the solve window_solve.hip, the LM iteration window_lm.hip
// (no reference counterpart: SURVEY s8 "new").
#include "runtime_internal.h"

extern "C" int sage_window_num_keyframes(const SageWindow *w) { return w ? w->K : 0; }
extern "C" int sage_window_num_links(const SageWindow *w) { return w ? (int)w->links.size() : 0; }
extern "C" int sage_window_block_size(const SageWindow *w) { return w ? w->B : 0; }
extern "C" int sage_window_solver_block_size(const SageWindow *w) { return w && w->finalized ? w->rows.Bs : 0; }
extern "C" size_t sage_window_packed_count(const SageWindow *w)
{
  if (!w)
    return 0;
  const size_t BB = (size_t)w->B * w->B;
  return (size_t)w->K * BB + w->links.size() * BB + (size_t)w->K * w->B + 4;
}
extern "C" double *sage_window_packed_dev(SageWindow *w) { return w ? w->packed.as<double>() : nullptr; }
extern "C" double *sage_window_error_dev(SageWindow *w) { return w ? w->errbuf.as<double>() : nullptr; }
extern "C" double sage_window_residuals_per_linearize(const SageWindow *w) { return w ? w->residuals_per_lin : 0; }
extern "C" double sage_window_bytes_per_linearize(const SageWindow *w) { return w ? w->bytes_per_lin : 0; }

std::vector<int32_t> window_link_pairs(const SageWindow *w)
{
  std::vector<int32_t> lk;
  for (const auto &l : w->links)
    lk.insert(lk.end(), {l.first, l.second});
  return lk;
}

int window_local_edge(const SageWindow *w, int global_edge)
{
  const auto it = std::lower_bound(w->local_edges.begin(), w->local_edges.end(), global_edge);
  return it != w->local_edges.end() && *it == global_edge ? (int)(it - w->local_edges.begin()) : -1;
}

bool window_owns_edge(const SageWindow *w, int global_edge)
{
  return std::binary_search(w->owned_edges.begin(), w->owned_edges.end(), global_edge);
}

bool window_has_holds(const SageWindow *w)
{
  return std::any_of(w->hold.begin(), w->hold.end(), [](uint8_t h) { return h != 0; });
}

int window_upload_vars(SageWindow *w, int set)
{
  if (w->dpt_set == set)
    w->dpt_set = -1;
  if (set == 0)
    ++w->vars_epoch; // whatever was linearised is no longer the system at the current variables
  std::vector<float> buf((size_t)w->K * w->VS, 0.f);
  for (int k = 0; k < w->K; ++k)
    w->hv.pack(set, k, w->cfg.CS, &buf[(size_t)k * w->VS]);
  SAGE_HIP(hipMemcpyAsync(w->vars[set].p, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream)); // buf is a temporary
  return SAGE_OK;
}

extern "C" int sage_window_get_keyframe(const SageWindow *w, int kf, float *pose12, float *code, float *scale)
{
  if (!w || kf < 0 || kf >= w->K)
    return SAGE_E_INVALID;
  if (pose12)
    std::memcpy(pose12, &w->hv.pose[0][(size_t)kf * 12], 12 * sizeof(float));
  if (code)
    std::memcpy(code, &w->hv.code[0][(size_t)kf * w->cfg.CS], w->cfg.CS * sizeof(float));
  if (scale)
    *scale = w->hv.scale[0][kf];
  return SAGE_OK;
}

extern "C" int sage_window_set_keyframe(SageWindow *w, int kf, const float *pose12, const float *code, float scale)
{
  if (!w || kf < 0 || kf >= w->K || !pose12 || !code)
    return SAGE_E_INVALID;
  (void)window_sync_candidate(w);
  for (int s = 0; s < 2; ++s)
  {
    std::memcpy(&w->hv.pose[s][(size_t)kf * 12], pose12, 12 * sizeof(float));
    std::memcpy(&w->hv.code[s][(size_t)kf * w->cfg.CS], code, w->cfg.CS * sizeof(float));
    w->hv.scale[s][kf] = scale;
  }
  if (w->finalized)
  {
    int rc;
    if ((rc = window_upload_vars(w, 0)) || (rc = window_upload_vars(w, 1)))
      return rc;
  }
  return SAGE_OK;
}
