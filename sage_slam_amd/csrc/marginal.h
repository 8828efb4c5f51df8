// marginal.h -- marginal priors (marginal_host.cpp, window_prior.hip): the handle a marginalisation leaves behind, and the
// layout of a window's prior terms as pure integer arithmetic (window_plan.h style): which structure-only links a term
// appends, where each block of its information matrix lands in the packed system, who owns it.  Standard library only -- no
// HIP, no environment.
//
// Convention (the window's): e(d) = e - 2 g^T d + d^T A d, step A d = g.  A prior over m keyframes holds Lambda [mB x mB],
// eta [mB], c and the point x0 it was linearised at; rows per keyframe in block order (pose 6, code CS, scale 1).  At
// variables x its term is  AtA = Lambda (constant: first-estimate Jacobians), Atb = eta - Lambda delta,
// err = delta^T Lambda delta - 2 eta^T delta + c,  delta_k = [pose_local(x0_k, x_k), code - code0, scale - scale0].
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "damped_system.h" // SAGE_HD

struct SageMarginalPrior
{
  int m = 0, CS = 0;
  std::vector<double> Lambda, eta; // [mB][mB], [mB]
  double c = 0.0;
  std::vector<float> pose, code, scale; // the linearisation point: [m][12], [m][CS], [m]
  std::vector<int32_t> kf;              // the ids its keyframes had in the window it came from
  int B() const { return 7 + CS; }
  int rows() const { return m * B(); }
};

namespace sage
{
namespace marg
{

constexpr int kMaxKeyframes = 16; // of one prior: the evaluation kernel keeps delta [16 * 39] in LDS
constexpr int kRowTile = 64;      // rows of a workgroup of the evaluation kernel

// 0 ok, -1 invalid (m < 1, an id outside [0, K), a duplicate), -2 unsupported (m above the cap): SAGE_OK / _E_INVALID / _E_UNSUPPORTED
inline int check_keyframes(int K, const int32_t *kf, int m)
{
  if (m > kMaxKeyframes)
    return -2;
  if (m < 1 || !kf)
    return -1;
  for (int i = 0; i < m; ++i)
  {
    if (kf[i] < 0 || kf[i] >= K)
      return -1;
    for (int j = 0; j < i; ++j)
      if (kf[j] == kf[i])
        return -1;
  }
  return 0;
}

// ---- a window's local prior terms as the kernels of window_prior.hip see them ----
struct PriorTermDev // a row of the table: one local term
{
  int32_t m, n;               // keyframes, rows (m B)
  int32_t kf[kMaxKeyframes];  // the window's keyframes behind the prior's
  int32_t tile0;              // its first row tile among all terms' (the partials' index)
  int32_t pad;
  size_t lam, vec, x0;        // offsets: Lambda (doubles), eta / Atb (doubles), the linearisation point (floats, [m][VS] as a window's variables)
  double c;
};
struct PriorGradRow // rows [src, src + B) of the terms' Atb are added to keyframe kf's gradient
{
  int32_t kf, pad;
  size_t src;
};

// a term's error from its row tiles' partials {delta^T Lambda delta, eta^T delta}: c first, then tile by tile -- the one
// order the add kernel, the error pass's totals and the host copy share
SAGE_HD inline double prior_term_error(const PriorTermDev &t, const double *part)
{
  double e = t.c;
  for (int tile = 0; tile * kRowTile < t.n; ++tile)
    e += part[2 * (t.tile0 + tile)] - 2.0 * part[2 * (t.tile0 + tile) + 1];
  return e;
}
SAGE_HD inline double prior_error_total(const PriorTermDev *table, int n_terms, const double *part)
{
  double e = 0.0;
  for (int t = 0; t < n_terms; ++t)
    e += prior_term_error(table[t], part);
  return e;
}

// the assembly's column map (window_eval.hip: edge_col; capi.edge_col): row bi of a keyframe's block (pose 6, code CS, scale)
// -> column of a per-edge system of column map `type` (0 photometric, 1 geometric, 2 poses and scales only) for the keyframe
// in `role` (0 source, 1 destination); -1: absent
constexpr int packed_col(int type, int role, int bi, int CS)
{
  if (bi < 6)
    return role * 6 + bi;
  if (type == 2)
    return bi == 6 + CS ? 12 + role : -1;
  if (type == 0)
    return role == 1 ? -1 : (bi < 6 + CS ? 12 + (bi - 6) : 12 + CS);
  return bi < 6 + CS ? 12 + role * CS + (bi - 6) : 12 + 2 * CS + role;
}

typedef std::vector<std::pair<int, int>> Links; // (a, b), a < b

inline int find_link(const Links &links, int a, int b)
{
  const std::pair<int, int> want(std::min(a, b), std::max(a, b));
  for (size_t l = 0; l < links.size(); ++l)
    if (links[l] == want)
      return (int)l;
  return -1;
}

// the pairs of a prior's keyframes no link joins yet, ascending (a, b): the structure-only links the term appends
inline Links missing_links(const Links &links, const int32_t *kf, int m)
{
  Links out;
  for (int i = 0; i < m; ++i)
    for (int j = i + 1; j < m; ++j)
      if (find_link(links, kf[i], kf[j]) < 0)
        out.emplace_back(std::min(kf[i], kf[j]), std::max(kf[i], kf[j]));
  std::sort(out.begin(), out.end());
  return out;
}

// block (i, j), i <= j, of term `term`'s Lambda -> packed block `block` (a keyframe's diagonal block: its id; a link block:
// K + link).  A link block is [row in the older keyframe][column in the newer]: transposed = the prior orders the pair the
// other way round, Lambda_ij^T is what lands there
struct Placement
{
  int term, i, j, block;
  bool transposed;
};
struct GradEntry // rows [pos B, (pos + 1) B) of term `term`'s Atb go to keyframe kf's gradient
{
  int kf, term, pos;
};
struct PriorLayout
{
  std::vector<int> local;       // this rank's terms, ascending term id: every term on rank 0, none elsewhere
  std::vector<Placement> place; // block-major (ascending packed block), each block's in term-id order
  std::vector<int> blocks;      // the distinct packed blocks, ascending
  std::vector<GradEntry> grad;  // keyframe-major, each keyframe's in term-id order
  int missing = 0;              // pairs without a link: the layout is void (add_prior_term appends them, so: 0)
};

inline bool rank_owns_priors(int rank) { return rank == 0; } // like a scale-prior graph term

inline PriorLayout prior_layout(int K, const Links &links, const std::vector<std::vector<int32_t>> &kf_maps, int rank)
{
  PriorLayout L;
  if (!rank_owns_priors(rank))
    return L;
  for (size_t t = 0; t < kf_maps.size(); ++t)
  {
    const std::vector<int32_t> &kf = kf_maps[t];
    const int m = (int)kf.size();
    L.local.push_back((int)t);
    for (int i = 0; i < m; ++i)
    {
      L.place.push_back(Placement{(int)t, i, i, kf[i], false});
      L.grad.push_back(GradEntry{kf[i], (int)t, i});
      for (int j = i + 1; j < m; ++j)
      {
        const int l = find_link(links, kf[i], kf[j]);
        if (l < 0)
          ++L.missing;
        else
          L.place.push_back(Placement{(int)t, i, j, K + l, kf[i] > kf[j]});
      }
    }
  }
  std::stable_sort(L.place.begin(), L.place.end(), [](const Placement &a, const Placement &b) { return a.block < b.block; });
  std::stable_sort(L.grad.begin(), L.grad.end(), [](const GradEntry &a, const GradEntry &b) { return a.kf < b.kf; });
  for (const Placement &p : L.place)
    if (L.blocks.empty() || L.blocks.back() != p.block)
      L.blocks.push_back(p.block);
  return L;
}

// the image of the local terms' Lambda in the packed layout: per entry of L.blocks its B x B doubles, the blocks that land
// there summed in term-id order
inline std::vector<double> prior_image(const PriorLayout &L, int B, const std::vector<const double *> &Lambda, const std::vector<int> &m)
{
  const size_t BB = (size_t)B * B;
  std::vector<double> img(L.blocks.size() * BB, 0.0);
  size_t slot = 0;
  for (const Placement &p : L.place)
  {
    while (L.blocks[slot] != p.block)
      ++slot;
    const double *Lam = Lambda[p.term];
    const size_t n = (size_t)m[p.term] * B;
    double *dst = &img[slot * BB];
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c)
        dst[(size_t)r * B + c] += p.transposed ? Lam[((size_t)p.j * B + r) * n + (size_t)p.i * B + c]
                                               : Lam[((size_t)p.i * B + r) * n + (size_t)p.j * B + c];
  }
  return img;
}

} // namespace marg
} // namespace sage
