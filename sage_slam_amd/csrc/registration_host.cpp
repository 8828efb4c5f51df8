// registration_host.cpp -- (no HIP) the host side of robust registration (include/sage_ba.h): sage_tls_estimate,
// sage_registration_finish, and the layout of a batch of votes (registration_batch_plan, sage_robust_registration_batch_plan).  teaser::RobustRegistrationSolver::solve for the chain graph without inlier selection
// (thirdparty/TEASER-plusplus/teaser/src/registration.cc:586-690), from the scale on:
//   the chain TIMs i -> i + 1 (the last one wraps to 0), their bounds nb_leaf + nb_root, both dst side and bounds over scale
//   the GNC's scalar bound: noise_bound * (2 / scale) (:648-650), squared, < 1e-16 -> 1e-2 (:1022-1025)
//   GNC-TLS with per-TIM bounds as written (:990-1101): svdRot with the weights, squared residuals, at iteration 0
//     mu = 1 / (2 max / bound^2 - 1) and the exit at mu <= 0, the closed-form weights, the cost of the PREVIOUS weights, the
//     exit at |cost - previous| < threshold; the mask is weight >= 0.5
//   the translation: per axis one scalar vote (ScalarTLSEstimator::estimate, :21-88) over dst - scale R src with the bounds
//     nb sqrt(cbar2) (:361-388), and the AND of the three masks
// All in fp64, sums sequential in the reference's order.  svdRot's 3x3 SVD (registration_math.h, shared with the device
// finish, reg_finish_kernel in registration.hip) is a one-sided Jacobi here (Eigen's JacobiSVD
// there): V diag(1, 1, det U det V) U^T is the same matrix whenever H has rank >= 2; at rank 1 (N = 2: the two chain TIMs
// are antiparallel) the rotation about the one direction is open in both, and each picks its own.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <utility>
#include <vector>

#include "registration_math.h"
#include "registration_plan.h"
#include "sage_ba.h"

namespace
{
using sage_reg::Mat3;

// utils.h:121-136: H = X diag(W) Y^T, R = V U^T with V's last column negated when det U det V < 0 (registration_math.h)
Mat3 svd_rot(const std::vector<double> &X, const std::vector<double> &Y, const std::vector<double> &W, int n)
{
  Mat3 H;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
    {
      double s = 0.0;
      for (int i = 0; i < n; ++i)
        s += (X[3 * i + r] * W[i]) * Y[3 * i + c];
      H.m[r][c] = s;
    }
  return sage_reg::svd_rot_of(H);
}

bool params_ok(const SageRegistrationParams *p)
{
  return p && std::isfinite(p->noise_bound) && p->noise_bound > 0 && std::isfinite(p->cbar2) && p->cbar2 > 0 &&
         p->rotation_max_iterations >= 0 && std::isfinite(p->rotation_cost_threshold) && std::isfinite(p->rotation_gnc_factor) &&
         p->rotation_gnc_factor > 1 && p->rotation_tim_graph >= SAGE_REG_CHAIN && p->rotation_tim_graph <= SAGE_REG_COMPLETE &&
         p->inlier_selection_mode >= SAGE_REG_SELECT_PMC_EXACT && p->inlier_selection_mode <= SAGE_REG_SELECT_NONE &&
         p->rotation_algorithm >= SAGE_REG_GNC_TLS && p->rotation_algorithm <= SAGE_REG_FGR;
}
} // namespace

// SAGE_OK, SAGE_E_INVALID or SAGE_E_UNSUPPORTED for a parameter set (shared with registration.hip: runtime_internal.h)
int registration_check_params(const SageRegistrationParams *p)
{
  if (!params_ok(p))
    return SAGE_E_INVALID;
  if (p->rotation_tim_graph != SAGE_REG_CHAIN || p->inlier_selection_mode != SAGE_REG_SELECT_NONE ||
      p->rotation_algorithm != SAGE_REG_GNC_TLS)
    return SAGE_E_UNSUPPORTED;
  return SAGE_OK;
}

// ---- the layout of a batch of votes (registration_plan.h) ----
int registration_sort_tile()
{
  if (const char *env = std::getenv("SAGE_REG_SORT_TILE")) // measurement: scripts/registration_bench.py times the three sizes
  {
    const int v = std::atoi(env);
    if (v == 1024 || v == 2048 || v == 4096)
      return v;
  }
  return 1024;
}

int registration_sort_launches(int P, int tile)
{
  int n = 1; // the stages up to the tile, in LDS
  for (int k = 2 * tile; k <= P; k <<= 1)
  {
    int n_global = 0; // the distances k / 2 .. tile: two per launch, an odd one out alone; then the tile's in LDS
    for (int q = k >> 1; q >= tile; q >>= 1)
      ++n_global;
    n += (n_global + 1) / 2 + 1;
  }
  return n;
}

void registration_batch_plan(const int32_t *N, int B, int sort_tile, RegBatchPlan *plan)
{
  *plan = RegBatchPlan();
  plan->sort_tile = sort_tile;
  int n = 0;
  for (int b = 0; b < B; ++b)
  {
    if (N[b] < 2)
      continue; // (does not vote: no segment, no record, no launch)
    RegBatchSegment &s = plan->seg[n++];
    s.row = b;
    s.N = N[b];
    s.pairs = N[b] * (N[b] - 1) / 2;
    s.P = 4096;
    while (s.P < 2 * s.pairs)
      s.P <<= 1;
    s.n_tiles = (2 * s.pairs + 2047) / 2048;
  }
  plan->n = n;
  // descending P, rows of equal P in the caller's order: every segment then starts at a multiple of its own P
  std::stable_sort(plan->seg, plan->seg + n, [](const RegBatchSegment &a, const RegBatchSegment &b) { return a.P > b.P; });
  int64_t rows = 16 * (int64_t)n, record = 0;
  for (int i = 0; i < n; ++i)
  {
    RegBatchSegment &s = plan->seg[i];
    s.start = plan->endpoints;
    s.pair0 = plan->pairs;
    s.tile0 = plan->tiles;
    s.cblock0 = plan->cblocks;
    s.rows0 = rows;
    s.record0 = record;
    plan->endpoints += s.P;
    plan->pairs += s.pairs;
    plan->tiles += s.n_tiles;
    plan->cblocks += (s.pairs + 255) / 256;
    rows += 160 * (int64_t)(s.P / 2048) + 64;
    record += 64 + 32 * (int64_t)s.N;
  }
  plan->keys_bytes = 8 * (int64_t)plan->endpoints;
  plan->payload_bytes = 4 * (int64_t)plan->endpoints;
  plan->pairs_bytes = 16 * (int64_t)plan->pairs;
  plan->tiles_bytes = rows;
  plan->device_bytes = plan->keys_bytes + plan->payload_bytes + plan->pairs_bytes + plan->tiles_bytes;
  plan->pinned_bytes = record;
  // (one voting problem: the single call's path, whose publish kernel posts the ticket)
  plan->launches = n ? registration_sort_launches(plan->seg[0].P, sort_tile) + (n == 1 ? kRegSingleFixedLaunches : kRegBatchFixedLaunches) : 0;
}

extern "C" int sage_robust_registration_batch_plan(const int32_t *N, int B, int64_t *device_bytes, int64_t *pinned_bytes,
                                                   int32_t *launches, int32_t *order)
{
  if (B < 0 || B > SAGE_REG_MAX_BATCH || (B > 0 && !N))
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
    if (N[b] < 0 || N[b] > SAGE_REG_MAX_POINTS)
      return SAGE_E_INVALID;
  RegBatchPlan plan;
  registration_batch_plan(N, B, registration_sort_tile(), &plan);
  if (device_bytes)
    *device_bytes = plan.device_bytes;
  if (pinned_bytes)
    *pinned_bytes = plan.pinned_bytes;
  if (launches)
    *launches = plan.launches;
  if (order)
    for (int b = 0; b < B; ++b)
      order[b] = b < plan.n ? plan.seg[b].row : -1;
  return SAGE_OK;
}

extern "C" int sage_registration_finish_plan(const int32_t *N, int B, int32_t *launches, int64_t *pinned_bytes, int32_t *lds_bytes,
                                             int32_t *workgroups)
{
  if (B < 0 || B > SAGE_REG_MAX_BATCH || (B > 0 && !N))
    return SAGE_E_INVALID;
  for (int b = 0; b < B; ++b)
    if (N[b] < 0 || N[b] > SAGE_REG_MAX_POINTS)
      return SAGE_E_INVALID;
  RegBatchPlan plan;
  registration_batch_plan(N, B, registration_sort_tile(), &plan);
  int64_t pinned = plan.pinned_bytes;
  for (int i = 0; i < plan.n; ++i)
    pinned += reg_finish_record_bytes(plan.seg[i].N);
  if (launches)
    *launches = plan.n ? plan.launches + 1 : 0;
  if (pinned_bytes)
    *pinned_bytes = pinned;
  if (lds_bytes)
    *lds_bytes = plan.n ? kRegFinishLdsBytes : 0;
  if (workgroups)
    *workgroups = plan.n;
  return SAGE_OK;
}

extern "C" int sage_tls_estimate(const double *X, const double *ranges, int n, double *estimate, uint8_t *inliers)
{
  if (!X || !ranges || n < 1)
    return SAGE_E_INVALID;
  std::vector<std::pair<double, int>> h;
  h.reserve(2 * (size_t)n);
  for (int i = 0; i < n; ++i)
  {
    h.push_back(std::make_pair(X[i] - ranges[i], i + 1));
    h.push_back(std::make_pair(X[i] + ranges[i], -i - 1));
  }
  // (std::sort there: the order of equal values is open; stable here.  The comparison sees the values alone, as there)
  std::stable_sort(h.begin(), h.end(), [](const std::pair<double, int> &a, const std::pair<double, int> &b) { return a.first < b.first; });
  double ranges_inverse_sum = 0.0;
  for (int i = 0; i < n; ++i)
    ranges_inverse_sum += ranges[i];
  double dot_X_weights = 0, dot_weights_consensus = 0, sum_xi = 0, sum_xi_square = 0;
  int consensus_set_cardinal = 0;
  double best_cost = std::numeric_limits<double>::quiet_NaN(), best_x = std::numeric_limits<double>::quiet_NaN();
  bool have = false;
  for (size_t k = 0; k < h.size(); ++k)
  {
    const int idx = std::abs(h[k].second) - 1;
    const int epsilon = h[k].second > 0 ? 1 : -1;
    const double weight = 1.0 / (ranges[idx] * ranges[idx]);
    consensus_set_cardinal += epsilon;
    dot_weights_consensus += epsilon * weight;
    dot_X_weights += epsilon * weight * X[idx];
    ranges_inverse_sum -= epsilon * ranges[idx];
    sum_xi += epsilon * X[idx];
    sum_xi_square += epsilon * X[idx] * X[idx];
    const double x_hat = dot_X_weights / dot_weights_consensus;
    const double residual = consensus_set_cardinal * x_hat * x_hat + sum_xi_square - 2 * sum_xi * x_hat;
    const double cost = residual + ranges_inverse_sum;
    // minCoeff: the first smallest; a NaN never wins (all NaN: the estimate is NaN)
    if (cost == cost && (!have || cost < best_cost))
    {
      best_cost = cost;
      best_x = x_hat;
      have = true;
    }
  }
  if (estimate)
    *estimate = best_x;
  if (inliers)
    for (int i = 0; i < n; ++i)
      inliers[i] = std::fabs(X[i] - best_x) <= ranges[i] ? 1 : 0;
  return SAGE_OK;
}

extern "C" int sage_registration_finish(const float *src_f, const float *dst_f, const float *nb_f, int N, double scale,
                                        const SageRegistrationParams *p, SageRegistrationResult *res, int32_t *inliers_host,
                                        uint8_t *rotation_mask)
{
  if (!src_f || !dst_f || !nb_f || !res || N < 2 || N > SAGE_REG_MAX_POINTS)
    return SAGE_E_INVALID;
  if (int rc = registration_check_params(p))
    return rc;
  const int n = N;
  std::vector<double> src(3 * (size_t)n), dst(3 * (size_t)n), nb(n);
  for (int i = 0; i < 3 * n; ++i)
  {
    src[i] = (double)src_f[i];
    dst[i] = (double)dst_f[i];
  }
  for (int i = 0; i < n; ++i)
    nb[i] = (double)nb_f[i];

  // the chain TIMs, scale removed from the dst side (pruned_dst_tims_ *= 1 / scale)
  const double inv_scale = 1 / scale;
  std::vector<double> ts(3 * (size_t)n), td(3 * (size_t)n), tb(n), bsq(n);
  for (int i = 0; i < n; ++i)
  {
    const int leaf = i != n - 1 ? i + 1 : 0;
    for (int c = 0; c < 3; ++c)
    {
      ts[3 * i + c] = src[3 * leaf + c] - src[3 * i + c];
      td[3 * i + c] = (dst[3 * leaf + c] - dst[3 * i + c]) * inv_scale;
    }
    tb[i] = (nb[leaf] + nb[i]) * inv_scale;
    bsq[i] = tb[i] * tb[i];
  }
  const double gnc_bound = p->noise_bound * (2 / scale);
  double noise_bound_sq = std::pow(gnc_bound, 2);
  if (noise_bound_sq < 1e-16)
    noise_bound_sq = 1e-2;

  std::vector<double> weights(n, 1.0), residuals_sq(n);
  Mat3 R = {{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
  double mu = 1, prev_cost = std::numeric_limits<double>::infinity();
  int it = 0;
  for (; it < p->rotation_max_iterations; ++it)
  {
    R = svd_rot(ts, td, weights, n);
    for (int j = 0; j < n; ++j)
    {
      double s = 0.0;
      for (int r = 0; r < 3; ++r)
      {
        const double d = td[3 * j + r] - (R.m[r][0] * ts[3 * j + 0] + R.m[r][1] * ts[3 * j + 1] + R.m[r][2] * ts[3 * j + 2]);
        s += d * d;
      }
      residuals_sq[j] = s;
    }
    if (it == 0)
    {
      const double max_residual = *std::max_element(residuals_sq.begin(), residuals_sq.end());
      mu = 1 / (2 * max_residual / noise_bound_sq - 1);
      if (mu <= 0)
        break;
    }
    double cost = 0;
    for (int j = 0; j < n; ++j)
    {
      const double th1 = (mu + 1) / mu * bsq[j], th2 = mu / (mu + 1) * bsq[j];
      cost += weights[j] * residuals_sq[j];
      if (residuals_sq[j] >= th1)
        weights[j] = 0;
      else if (residuals_sq[j] <= th2)
        weights[j] = 1;
      else
        weights[j] = std::sqrt(bsq[j] * mu * (mu + 1) / residuals_sq[j]) - mu;
    }
    const double cost_diff = std::fabs(cost - prev_cost);
    mu = mu * p->rotation_gnc_factor;
    prev_cost = cost;
    if (cost_diff < p->rotation_cost_threshold)
      break;
  }
  int n_rot = 0;
  for (int i = 0; i < n; ++i)
  {
    const uint8_t in = weights[i] >= 0.5 ? 1 : 0;
    n_rot += in;
    if (rotation_mask)
      rotation_mask[i] = in;
  }

  // the translation: dst - scale R src per axis
  std::vector<double> raw(n), alphas(n);
  std::vector<uint8_t> mask(n, 1), axis_mask(n);
  const double sq = std::sqrt(p->cbar2);
  for (int i = 0; i < n; ++i)
    alphas[i] = nb[i] * sq;
  Mat3 sR;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      sR.m[r][c] = scale * R.m[r][c];
  for (int r = 0; r < 3; ++r)
  {
    for (int i = 0; i < n; ++i)
      raw[i] = dst[3 * i + r] - (sR.m[r][0] * src[3 * i + 0] + sR.m[r][1] * src[3 * i + 1] + sR.m[r][2] * src[3 * i + 2]);
    sage_tls_estimate(raw.data(), alphas.data(), n, &res->t[r], axis_mask.data());
    for (int i = 0; i < n; ++i)
      mask[i] = mask[i] & axis_mask[i];
  }
  int n_in = 0;
  for (int i = 0; i < n; ++i)
    if (mask[i])
    {
      if (inliers_host)
        inliers_host[n_in] = i;
      ++n_in;
    }
  res->valid = 1;
  res->scale = scale;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      res->R[3 * r + c] = R.m[r][c];
  res->n_inliers = n_in;
  res->rotation_iterations = it;
  res->n_rotation_inliers = n_rot;
  return SAGE_OK;
}
