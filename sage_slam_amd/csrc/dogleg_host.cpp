// dogleg_host.cpp -- (no HIP) Powell's dogleg as the reference's ISAM2 runs it: the dogleg point, the trust-region policy
// around an evaluation callback, and the incidence lists of the product kernels.  gtsam's statement of the algorithm is
// thirdparty/gtsam/gtsam/nonlinear/DoglegOptimizerImpl.{h,cpp}; the lines are cited where a rule is taken from there.
#include <cmath>

#include "dogleg.h"
#include "sage_ba.h"

using namespace sage::dogleg;

extern "C" void sage_dogleg_config_default(SageDoglegConfig *cfg)
{
  if (!cfg)
    return;
  cfg->init_delta = 1.0;  // deepfactors.cpp:89 (ISAM2DoglegParams' initialDelta)
  cfg->min_delta = 1e-5;  // DoglegOptimizerImpl.h:213, :235
  cfg->mode = SAGE_DOGLEG_ONE_STEP_PER_ITERATION;
}

// With u = s g, s = g.g / g.Ag (optimizeGradientSearch): |u|^2 = s^2 g.g, u.n = s g.n
extern "C" int sage_dogleg_point(double delta, double gg, double gn, double nn, double gAg, double *a, double *b, int *region)
{
  if (!a || !b || !region)
    return SAGE_E_INVALID;
  *a = *b = 0.0;
  *region = 0;
  if (gg == 0.0) // the gradient vanishes: converged, the zero step
    return SAGE_OK;
  if (!(gAg > 0.0))
    return SAGE_E_NOT_PSD;
  const double s = gg / gAg;
  const double uu = s * s * gg, un = s * gn, d2 = delta * delta;
  if (d2 < uu) // DoglegOptimizerImpl.cpp:34-38: the steepest-descent point scaled to the radius
  {
    *a = std::sqrt(d2 / uu) * s;
    return SAGE_OK;
  }
  if (d2 < nn) // :39-41, ComputeBlend :51-83: the root of |(1 - tau) u + tau n| = delta in [0, 1]
  {
    const double qa = uu - 2.0 * un + nn, qb = 2.0 * (un - uu), qc = uu - d2;
    const double root = std::sqrt(qb * qb - 4.0 * qa * qc);
    const double tau1 = (-qb + root) / (2.0 * qa), tau2 = (-qb - root) / (2.0 * qa);
    const double tau = (0.0 <= tau1 && tau1 <= 1.0) ? tau1 : tau2;
    *a = (1.0 - tau) * s;
    *b = tau;
    *region = 1;
    return SAGE_OK;
  }
  *b = 1.0; // :42-46: the Gauss-Newton point lies inside the region
  *region = 2;
  return SAGE_OK;
}

extern "C" int sage_dogleg_iterate(const SageDoglegConfig *cfg, const double *dots, double f_error, SageDoglegEvalFn eval,
                                   void *ctx, SageDoglegState *st)
{
  if (!cfg || !dots || !eval || !st)
    return SAGE_E_INVALID;
  if (cfg->mode != SAGE_DOGLEG_SEARCH_EACH_ITERATION && cfg->mode != SAGE_DOGLEG_SEARCH_REDUCE_ONLY &&
      cfg->mode != SAGE_DOGLEG_ONE_STEP_PER_ITERATION)
    return SAGE_E_INVALID;
  double delta = st->delta > 0.0 ? st->delta : cfg->init_delta;
  double a = 0.0, b = 0.0, f_cand = f_error, rho = 0.5;
  int region = 0, evals = 0, rc; // (st is written at the end only: an error code leaves it untouched)
  const bool searching = cfg->mode == SAGE_DOGLEG_SEARCH_EACH_ITERATION;
  const bool one_step = cfg->mode == SAGE_DOGLEG_ONE_STEP_PER_ITERATION;
  enum { none, increased, decreased } last = none; // (Iterate :150: no alternating within one iteration)
  bool stay = dots[kGG] != 0.0;                     // a vanishing gradient: nothing to evaluate
  while (stay)
  {
    if ((rc = sage_dogleg_point(delta, dots[kGG], dots[kGN], dots[kNN], dots[kGAG], &a, &b, &region)))
      return rc;
    if ((rc = eval(ctx, a, b, &f_cand)))
      return rc;
    ++evals;
    const double f_dec = f_error - f_cand, m_dec = model_decrease(dots, a, b);
    rho = (std::fabs(f_dec) < 1e-15 || std::fabs(m_dec) < 1e-15) ? 0.5 : f_dec / m_dec; // :180-182
    if (rho >= 0.75) // :186-203
    {
      const double grown = std::fmax(delta, 3.0 * std::sqrt(step_norm2(dots, a, b)));
      if (!searching || std::fabs(grown - delta) < 1e-15 || last == decreased)
        stay = false;
      else
        last = increased;
      delta = grown;
    }
    else if (rho >= 0.25) // :205-207
      stay = false;
    else if (rho >= 0.0) // :209-228
    {
      const bool at_min = !(delta > cfg->min_delta);
      if (one_step || last == increased || at_min)
        stay = false;
      else
        last = decreased;
      if (!at_min)
        delta *= 0.5;
    }
    else // :230-245: the error rose (or is NaN)
    {
      if (delta > cfg->min_delta)
      {
        delta *= 0.5;
        last = decreased;
      }
      else
      {
        a = b = 0.0; // the zero step, the error kept
        f_cand = f_error;
        stay = false;
      }
    }
  }
  st->delta = delta;
  st->error = f_error;
  st->candidate_error = f_cand;
  st->rho = rho;
  st->a = a;
  st->b = b;
  st->region = region;
  st->step_norm = std::sqrt(step_norm2(dots, a, b));
  st->sd_norm = dots[kGG] != 0.0 ? std::fabs(dots[kGG] / dots[kGAG]) * std::sqrt(dots[kGG]) : 0.0;
  st->gn_norm = std::sqrt(dots[kNN]);
  st->accepted = (a != 0.0 || b != 0.0) ? 1 : 0;
  for (int i = 0; i < kDots; ++i)
    st->dots[i] = dots[i];
  st->evals = evals;
  st->iters += 1;
  return SAGE_OK;
}

extern "C" int sage_dogleg_incidence(int K, int nlinks, const int32_t *links, int32_t *offsets, int32_t *entries)
{
  if (K < 1 || nlinks < 0 || (nlinks > 0 && !links) || !offsets || !entries)
    return SAGE_E_INVALID;
  for (int l = 0; l < nlinks; ++l)
  {
    const int32_t a = links[2 * l], b = links[2 * l + 1];
    if (a < 0 || a >= K || b < 0 || b >= K || a == b)
      return SAGE_E_INVALID;
  }
  for (int k = 0; k <= K; ++k)
    offsets[k] = 0;
  for (int l = 0; l < nlinks; ++l)
  {
    ++offsets[links[2 * l] + 1];
    ++offsets[links[2 * l + 1] + 1];
  }
  for (int k = 0; k < K; ++k)
    offsets[k + 1] += offsets[k] + 1; // (+ 1: the diagonal block)
  // fill: the diagonal first, then the links in the order they were added; the running position of keyframe k is kept in
  // its diagonal entry's second slot until the end
  for (int k = 0; k < K; ++k)
  {
    entries[2 * offsets[k]] = k;
    entries[2 * offsets[k] + 1] = 1; // entries of k written so far
  }
  for (int l = 0; l < nlinks; ++l)
    for (int t = 0; t < 2; ++t)
    {
      const int32_t k = links[2 * l + t];
      const int32_t at = offsets[k] + entries[2 * offsets[k] + 1]++;
      entries[2 * at] = K + l;
      entries[2 * at + 1] = t;
    }
  for (int k = 0; k < K; ++k)
    entries[2 * offsets[k] + 1] = 0;
  return SAGE_OK;
}
