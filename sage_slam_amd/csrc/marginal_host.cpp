// marginal_host.cpp -- the host side of marginalisation (marginal.h): the Schur complement that turns a sub-system into a
// prior, the prior's handle, the host mirror of the device term (window_prior.hip) and the C view of the layout plan.
// Plain C++17, no HIP include.  The elimination runs here and not on the device: it happens once per slide on a few hundred
// unknowns, and a one-workgroup device factorisation of a system this size was measured 30x slower than host cores
// (solve_kernels.hip).  Neither host Cholesky of the library fits: the block solver factors fixed 24 / 40 blocks on an
// envelope for one right-hand side, host_math.cpp only tests an LDL^T for positivity -- so the dense one below is the
// library's only plain dense Cholesky.
#include "marginal.h"

#include <cmath>
#include <cstring>

#include "damped_system.h"
#include "sage_ba.h"

namespace
{

// in place: the lower triangle of A [n x n] becomes L, A = L L^T.  false: a pivot that is not positive (or not finite)
bool dense_cholesky(double *A, int n)
{
  for (int j = 0; j < n; ++j)
  {
    double d = A[(size_t)j * n + j];
    for (int k = 0; k < j; ++k)
      d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
    if (!(d > 0.0) || !std::isfinite(d))
      return false;
    const double l = std::sqrt(d);
    A[(size_t)j * n + j] = l;
    for (int i = j + 1; i < n; ++i)
    {
      double s = A[(size_t)i * n + j];
      for (int k = 0; k < j; ++k)
        s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
      A[(size_t)i * n + j] = s / l;
    }
  }
  return true;
}

// x <- L^-1 x (forward), x <- L^-T x (backward); x is one column with stride `ld`
void solve_lower(const double *L, int n, double *x, size_t ld)
{
  for (int i = 0; i < n; ++i)
  {
    double s = x[i * ld];
    for (int k = 0; k < i; ++k)
      s -= L[(size_t)i * n + k] * x[k * ld];
    x[i * ld] = s / L[(size_t)i * n + i];
  }
}
void solve_lower_t(const double *L, int n, double *x, size_t ld)
{
  for (int i = n - 1; i >= 0; --i)
  {
    double s = x[i * ld];
    for (int k = i + 1; k < n; ++k)
      s -= L[(size_t)k * n + i] * x[k * ld];
    x[i * ld] = s / L[(size_t)i * n + i];
  }
}

} // namespace

extern "C" int sage_schur_marginal(const double *A, const double *g, double e, int n, const int32_t *drop, int n_drop,
                                   double *Lambda, double *eta, double *c)
{
  if (!A || !g || n < 1 || n_drop < 0 || n_drop >= n || (n_drop > 0 && !drop) || !Lambda || !eta || !c)
    return SAGE_E_INVALID;
  std::vector<char> is_drop(n, 0);
  for (int i = 0; i < n_drop; ++i)
  {
    if (drop[i] < 0 || drop[i] >= n || is_drop[drop[i]])
      return SAGE_E_INVALID;
    is_drop[drop[i]] = 1;
  }
  std::vector<int> d, k;
  for (int i = 0; i < n; ++i)
    (is_drop[i] ? d : k).push_back(i);
  const int nd = (int)d.size(), nk = (int)k.size();
  auto sym = [A, n](int r, int col) { return 0.5 * (A[(size_t)r * n + col] + A[(size_t)col * n + r]); };
  // L L^T = A_dd;  X = A_dd^-1 [A_dk | g_d], one column per keep row and one for the gradient
  std::vector<double> Ldd((size_t)nd * nd), X((size_t)nd * (nk + 1));
  for (int i = 0; i < nd; ++i)
    for (int j = 0; j < nd; ++j)
      Ldd[(size_t)i * nd + j] = sym(d[i], d[j]);
  if (nd > 0 && !dense_cholesky(Ldd.data(), nd))
    return SAGE_E_NOT_PSD; // (nothing written)
  const size_t ld = (size_t)nk + 1;
  for (int i = 0; i < nd; ++i)
  {
    for (int j = 0; j < nk; ++j)
      X[i * ld + j] = sym(d[i], k[j]);
    X[i * ld + nk] = g[d[i]];
  }
  for (int j = 0; j <= nk; ++j)
  {
    solve_lower(Ldd.data(), nd, X.data() + j, ld);
    solve_lower_t(Ldd.data(), nd, X.data() + j, ld);
  }
  std::vector<double> S((size_t)nk * nk);
  for (int i = 0; i < nk; ++i)
    for (int j = 0; j < nk; ++j)
    {
      double s = 0.0;
      for (int q = 0; q < nd; ++q)
        s += sym(k[i], d[q]) * X[q * ld + j];
      S[(size_t)i * nk + j] = sym(k[i], k[j]) - s;
    }
  for (int i = 0; i < nk; ++i)
  {
    for (int j = 0; j < nk; ++j)
      Lambda[(size_t)i * nk + j] = 0.5 * (S[(size_t)i * nk + j] + S[(size_t)j * nk + i]);
    double s = 0.0;
    for (int q = 0; q < nd; ++q)
      s += sym(k[i], d[q]) * X[q * ld + nk];
    eta[i] = g[k[i]] - s;
  }
  double s = 0.0;
  for (int q = 0; q < nd; ++q)
    s += g[d[q]] * X[q * ld + nk];
  *c = e - s;
  return SAGE_OK;
}

// ---- the handle ----
extern "C" int sage_marginal_prior_create(int m, int CS, const double *Lambda, const double *eta, double c, const float *pose12,
                                          const float *code, const float *scale, const int32_t *kf_ids, SageMarginalPrior **out)
{
  if (!out || !Lambda || !eta || !pose12 || !code || !scale || m < 1 || CS < 1)
    return SAGE_E_INVALID;
  if (m > sage::marg::kMaxKeyframes || (CS != 16 && CS != 32))
    return SAGE_E_UNSUPPORTED;
  SageMarginalPrior *p = new SageMarginalPrior();
  p->m = m;
  p->CS = CS;
  const size_t n = (size_t)p->rows();
  p->Lambda.assign(Lambda, Lambda + n * n);
  p->eta.assign(eta, eta + n);
  p->c = c;
  p->pose.assign(pose12, pose12 + (size_t)m * 12);
  p->code.assign(code, code + (size_t)m * CS);
  p->scale.assign(scale, scale + m);
  p->kf.resize(m);
  for (int i = 0; i < m; ++i)
    p->kf[i] = kf_ids ? kf_ids[i] : i;
  *out = p;
  return SAGE_OK;
}

extern "C" int sage_marginal_prior_dims(const SageMarginalPrior *p, int *m, int *CS)
{
  if (!p)
    return SAGE_E_INVALID;
  if (m)
    *m = p->m;
  if (CS)
    *CS = p->CS;
  return SAGE_OK;
}

extern "C" int sage_marginal_prior_get(const SageMarginalPrior *p, double *Lambda, double *eta, double *c, float *pose12,
                                       float *code, float *scale)
{
  if (!p)
    return SAGE_E_INVALID;
  auto put = [](auto *dst, const auto &v) {
    if (dst)
      std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
  };
  put(Lambda, p->Lambda);
  put(eta, p->eta);
  if (c)
    *c = p->c;
  put(pose12, p->pose);
  put(code, p->code);
  put(scale, p->scale);
  return SAGE_OK;
}

extern "C" int sage_marginal_prior_keyframes(const SageMarginalPrior *p, int32_t *kf_ids)
{
  if (!p || !kf_ids)
    return SAGE_E_INVALID;
  std::memcpy(kf_ids, p->kf.data(), p->kf.size() * sizeof(int32_t));
  return SAGE_OK;
}

extern "C" void sage_marginal_prior_destroy(SageMarginalPrior *p) { delete p; }

// ---- the host mirror of prior_eval_kernel: the same delta (sage::pose_local is the kernel's own function), the products as
//      one serial sum each ----
extern "C" int sage_prior_evaluate(const SageMarginalPrior *p, const float *pose12, const float *code, const float *scale,
                                   double *delta, double *Atb, double *err)
{
  if (!p || !pose12 || !code || !scale)
    return SAGE_E_INVALID;
  const int m = p->m, CS = p->CS, B = p->B(), n = p->rows();
  std::vector<double> d((size_t)n);
  for (int k = 0; k < m; ++k)
  {
    double *dk = &d[(size_t)k * B];
    sage::pose_local(&p->pose[(size_t)k * 12], pose12 + (size_t)k * 12, dk);
    for (int i = 0; i < CS; ++i)
      dk[6 + i] = (double)code[(size_t)k * CS + i] - (double)p->code[(size_t)k * CS + i];
    dk[6 + CS] = (double)scale[k] - (double)p->scale[k];
  }
  double quad = 0.0, lin = 0.0;
  for (int i = 0; i < n; ++i)
  {
    double s = 0.0;
    for (int j = 0; j < n; ++j)
      s += p->Lambda[(size_t)j * n + i] * d[j];
    if (Atb)
      Atb[i] = p->eta[i] - s;
    quad += d[i] * s;
    lin += p->eta[i] * d[i];
  }
  if (delta)
    std::memcpy(delta, d.data(), (size_t)n * sizeof(double));
  if (err)
    *err = quad - 2.0 * lin + p->c;
  return SAGE_OK;
}

// ---- the layout plan as the tests see it: the terms added one after the other to a window of K keyframes and `links`, as
//      sage_window_add_prior_term adds them, then laid out for `rank`.  m [n_terms], kf_maps: the terms' maps one behind the
//      other.  append [.][2]: the structure-only links in the order they were appended (room for sum m (m - 1) / 2);
//      place [.][5]: term, i, j, packed block, transposed (room for sum m (m + 1) / 2); owned [n_terms] ----
extern "C" int sage_prior_term_plan(int K, int nlinks, const int32_t *links, int n_terms, const int32_t *m, const int32_t *kf_maps,
                                    int rank, int world, int32_t *append, int32_t *n_append, int32_t *place, int32_t *n_place,
                                    int32_t *owned)
{
  if (K < 1 || nlinks < 0 || (nlinks > 0 && !links) || n_terms < 0 || (n_terms > 0 && (!m || !kf_maps)) || world < 1 || rank < 0 ||
      rank >= world)
    return SAGE_E_INVALID;
  sage::marg::Links lk;
  for (int l = 0; l < nlinks; ++l)
    lk.emplace_back(std::min(links[2 * l], links[2 * l + 1]), std::max(links[2 * l], links[2 * l + 1]));
  std::vector<std::vector<int32_t>> maps;
  int na = 0;
  const int32_t *kf = kf_maps;
  for (int t = 0; t < n_terms; ++t)
  {
    if (const int rc = sage::marg::check_keyframes(K, kf, m[t]))
      return rc; // (SAGE_E_INVALID = -1, SAGE_E_UNSUPPORTED = -2)
    for (const auto &ab : sage::marg::missing_links(lk, kf, m[t]))
    {
      lk.push_back(ab);
      if (append)
      {
        append[2 * na] = ab.first;
        append[2 * na + 1] = ab.second;
      }
      ++na;
    }
    maps.emplace_back(kf, kf + m[t]);
    kf += m[t];
  }
  const sage::marg::PriorLayout L = sage::marg::prior_layout(K, lk, maps, rank);
  if (n_append)
    *n_append = na;
  if (n_place)
    *n_place = (int32_t)L.place.size();
  if (place)
    for (size_t i = 0; i < L.place.size(); ++i)
    {
      const sage::marg::Placement &p = L.place[i];
      const int32_t row[5] = {p.term, p.i, p.j, p.block, p.transposed ? 1 : 0};
      std::memcpy(place + 5 * i, row, sizeof(row));
    }
  if (owned)
    for (int t = 0; t < n_terms; ++t)
      owned[t] = sage::marg::rank_owns_priors(rank) ? 1 : 0;
  return SAGE_OK;
}
