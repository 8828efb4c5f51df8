// shard_solve.cpp -- domain-decomposed damped solve of a link-sharded window (multi-GPU).
//
// No reference counterpart (the reference is one GPU, ISAM2 on the host).  Link ranges are contiguous
// (sage_window_set_shard), so every rank's slice of the block-sparse normal equations is COMPLETE for the keyframes that
// only its own links touch ("interior" keyframes): it eliminates them locally and only the Schur complement on the
// keyframes shared with other ranks ("separators": ~3 per range boundary of a temporal window) crosses xGMI:
//
//   A = H + P + damp*diag(H + P)        H = sum_r H^(r) (per-rank edge sums), P = diagonal priors (owned by one rank each)
//   rank r:   C^(r) = A^(r)_SS - A_SI A_II^-1 A_IS ,  c^(r) = b^(r)_S - A_SI A_II^-1 b_I          (I = its interior)
//   all-reduce (sum, double) of the separator buffer [blocks of C | c | 8 tail doubles]
//   every rank: (sum_r C^(r)) d_S = sum_r c^(r)   (block-envelope Cholesky over the separators, identical on all ranks)
//   rank r:   d_I = A_II^-1 (b_I - A_IS d_S)
//
// Both steps run on the fixed-block Cholesky of the window solve (block_solver.cpp, blocks padded to 24 / 40, so B <= 40):
// the local system keeps the interior keyframes first and the rank's separators last, block_chol_partial factorises
// the interior rows and leaves C^(r) / c^(r) in the separator rows, block_chol_partial_back substitutes d_I; the
// separator system is a packed system for sage_block_solve.
//
// Payload at K = 64, 8 ranks, B = 39: 96 blocks + rhs = 1.2 MB instead of the 3.0 MB packed system; per-rank
// factorisation: 8 interior keyframes + the 21-keyframe separator system instead of all 64 keyframes.
// The result equals the single-rank solve of the summed system to rounding (tests/test_shard_schur.py, world 2/4/8;
// tests/test_sharded_reduce_gloo.py over gloo).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "block_solver.h"
#include "damped_system.h"
#include "host_math.h"
#include "sage_ba.h"

struct SageShardPlan
{
  int K = 0, B = 0, rank = 0, world = 1, nlinks = 0;
  std::vector<std::pair<int, int>> links;
  std::vector<int> link_lo;        // [world + 1] link range of every rank
  std::vector<int> kf_owner;       // designated owner (lowest rank touching the keyframe; -1: untouched)
  std::vector<int> kf_ntouch;      // number of ranks touching the keyframe
  std::vector<int> sep_all;        // separator keyframes (touched by >= 2 ranks), ascending
  std::vector<int> sep_index;      // keyframe -> index in sep_all, or -1
  std::vector<int> interior;       // this rank's interior keyframes, ascending
  std::vector<int> sep_local;      // indices into sep_all of the separators this rank touches
  std::vector<int> local_links;    // links this rank owns
  // separator buffer = the packed layout of sage_block_solve over the separator keyframes: [diag blocks | blocks of the
  // coupled pairs i < j (rows i, cols j) | rhs | 8 tail doubles]; pair_block maps (i <= j) -> block index
  std::map<std::pair<int, int>, int> pair_block;
  std::vector<int32_t> sep_pairs;  // flat (i, j), i < j, in block order: the "links" of the separator system
  int n_pair_blocks = 0;
  size_t sep_doubles = 0;
  std::vector<int> int_pos;        // keyframe -> position among interior, or -1
  bool have_factor = false;        // eliminate() has left a factor for solve()
  bool assembled = false;          // domains of one assembled system (sage_shard_plan_create_domains)
  // local block system on the fixed-block kernels of the window solve (block size padded to Bp = 8 / 24 / 40): the interior
  // keyframes at positions [0, nI) (elimination order) and this rank's separators at [nI, nI + nS)
  int Bp = 0, nloc = 0, nblk = 0;
  std::vector<int32_t> row_first, row_off;
  std::vector<double> T, X, yv;
};

namespace
{
inline int touch_rank_range(const SageShardPlan &p, int link)
{
  // rank owning `link` (ranges are contiguous and ordered)
  int r = (int)(std::upper_bound(p.link_lo.begin(), p.link_lo.end(), link) - p.link_lo.begin()) - 1;
  return std::min(std::max(r, 0), p.world - 1);
}
} // namespace

// mode-independent part of the plan: given, for every link, the domain (rank) that assembles it, and for every keyframe
// whether it is a separator and who owns its prior
static int finish_plan(SageShardPlan *p, const std::vector<int> &link_dom, const std::vector<char> &is_sep)
{
  const int K = p->K, world = p->world, rank = p->rank;
  p->Bp = sage::padded_block(p->B); // the fixed-block kernels' padded block size
  if (p->Bp == 0)
    return SAGE_E_UNSUPPORTED;
  // touch[r][k]: domain r couples keyframe k through its interior (Schur fill: all separators a domain touches become
  // mutually coupled).  Assembled mode: a link between two separators is just that one block, not a reason for fill.
  std::vector<std::vector<char>> touch(world, std::vector<char>(K, 0));
  std::vector<std::pair<int, int>> direct_pairs;
  for (int l = 0; l < p->nlinks; ++l)
  {
    const int a = p->links[l].first, b = p->links[l].second;
    if (p->assembled && is_sep[a] && is_sep[b])
      direct_pairs.push_back({a, b});
    else
      touch[link_dom[l]][a] = touch[link_dom[l]][b] = 1;
  }
  p->sep_index.assign(K, -1);
  p->int_pos.assign(K, -1);
  for (int k = 0; k < K; ++k)
  {
    if (is_sep[k])
    {
      p->sep_index[k] = (int)p->sep_all.size();
      p->sep_all.push_back(k);
    }
    else if (p->kf_owner[k] == rank)
    {
      p->int_pos[k] = (int)p->interior.size();
      p->interior.push_back(k);
    }
  }
  for (int l = 0; l < p->nlinks; ++l)
    if (link_dom[l] == rank)
      p->local_links.push_back(l);
  // elimination order of the interior: ascending keyframe index, i.e. a temporal chain keeps its block band of 3.  The
  // rows of the separators BEHIND a piece of chain are short; those of the separators in FRONT of it fill across the
  // piece (3 GEMMs per block column).  Ordering a piece from its middle outwards would keep both short but doubles the
  // band (6 instead of 3): 24 instead of 7.5 block operations per interior row -- measured slower for every piece length.
  for (size_t i = 0; i < p->interior.size(); ++i)
    p->int_pos[p->interior[i]] = (int)i;
  for (size_t s = 0; s < p->sep_all.size(); ++s)
    if (touch[rank][p->sep_all[s]] || (p->assembled && rank == 0))
      p->sep_local.push_back((int)s);
  // coupled separator pairs: every domain couples all the separators it touches with each other (Schur fill through
  // its interior, direct links); identical on every rank
  for (int r = 0; r < world; ++r)
  {
    std::vector<int> sl;
    for (size_t s = 0; s < p->sep_all.size(); ++s)
      if (touch[r][p->sep_all[s]])
        sl.push_back((int)s);
    for (size_t i = 0; i < sl.size(); ++i)
      for (size_t j = i; j < sl.size(); ++j)
        p->pair_block.emplace(std::make_pair(sl[i], sl[j]), 0);
  }
  for (const auto &dp : direct_pairs)
  {
    const int i = p->sep_index[dp.first], j = p->sep_index[dp.second];
    p->pair_block.emplace(std::make_pair(std::min(i, j), std::max(i, j)), 0);
  }
  int nb = (int)p->sep_all.size(); // diagonal blocks first
  for (auto &kv : p->pair_block)
  {
    if (kv.first.first == kv.first.second)
      kv.second = kv.first.first;
    else
    {
      kv.second = nb++;
      p->sep_pairs.push_back(kv.first.first);
      p->sep_pairs.push_back(kv.first.second);
    }
  }
  for (int s = 0; s < (int)p->sep_all.size(); ++s)
    p->pair_block.emplace(std::make_pair(s, s), s);
  p->n_pair_blocks = nb;
  p->sep_doubles = (size_t)nb * p->B * p->B + p->sep_all.size() * (size_t)p->B + 8;
  // ---- block envelope of the local system
  const int nI = (int)p->interior.size(), nS = (int)p->sep_local.size();
  p->nloc = nI + nS;
  std::vector<int> lpos(K, -1);
  for (int i = 0; i < nI; ++i)
    lpos[p->interior[i]] = i;
  for (int i = 0; i < nS; ++i)
    lpos[p->sep_all[p->sep_local[i]]] = nI + i;
  p->row_first.resize(p->nloc);
  for (int q = 0; q < p->nloc; ++q)
    p->row_first[q] = q;
  for (int l : p->local_links)
  {
    const int a = lpos[p->links[l].first], b = lpos[p->links[l].second];
    if (a < 0 || b < 0)
      return SAGE_E_STATE;
    p->row_first[std::max(a, b)] = std::min(p->row_first[std::max(a, b)], (int32_t)std::min(a, b));
  }
  // a separator row receives fill from every earlier separator that shares interior columns with it: keep the
  // separator rows' envelopes contiguous down to the first interior column any of them reaches
  p->row_off.resize(p->nloc);
  int nb2 = 0;
  for (int q = 0; q < p->nloc; ++q)
  {
    p->row_off[q] = nb2;
    nb2 += q - p->row_first[q] + 1;
  }
  p->nblk = nb2;
  p->T.assign((size_t)nb2 * p->Bp * p->Bp, 0.0);
  p->X.assign((size_t)p->nloc * p->Bp * p->Bp, 0.0);
  p->yv.assign((size_t)p->nloc * p->Bp, 0.0);
  return SAGE_OK;
}

static SageShardPlan *new_plan(int K, int nlinks, const int32_t *links, int B, int rank, int world)
{
  SageShardPlan *p = new SageShardPlan;
  p->K = K; p->B = B; p->rank = rank; p->world = world; p->nlinks = nlinks;
  p->links.resize(nlinks);
  for (int l = 0; l < nlinks; ++l)
  {
    const int a = links[2 * l], b = links[2 * l + 1];
    if (a < 0 || b <= a || b >= K)
    {
      delete p;
      return nullptr;
    }
    p->links[l] = {a, b};
  }
  return p;
}

extern "C" int sage_shard_plan_create(int K, int nlinks, const int32_t *links, int B, int rank, int world,
                                      SageShardPlan **out)
{
  if (!out || K < 1 || B < 1 || nlinks < 0 || (nlinks > 0 && !links) || world < 1 || rank < 0 || rank >= world)
    return SAGE_E_INVALID;
  SageShardPlan *p = new_plan(K, nlinks, links, B, rank, world);
  if (!p)
    return SAGE_E_INVALID;
  p->link_lo.resize(world + 1);
  for (int r = 0; r <= world; ++r)
    p->link_lo[r] = (int)((long long)nlinks * r / world); // the rule of sage_window_set_shard
  std::vector<int> link_dom(nlinks);
  std::vector<std::vector<char>> touch(world, std::vector<char>(K, 0));
  for (int l = 0; l < nlinks; ++l)
  {
    link_dom[l] = touch_rank_range(*p, l);
    touch[link_dom[l]][p->links[l].first] = touch[link_dom[l]][p->links[l].second] = 1;
  }
  p->kf_owner.assign(K, -1);
  p->kf_ntouch.assign(K, 0);
  std::vector<char> is_sep(K, 0);
  for (int k = 0; k < K; ++k)
  {
    for (int r = 0; r < world; ++r)
      if (touch[r][k])
      {
        if (p->kf_owner[k] < 0)
          p->kf_owner[k] = r;
        p->kf_ntouch[k] += 1;
      }
    if (p->kf_owner[k] < 0)
      p->kf_owner[k] = 0; // a keyframe no link touches: a prior-only interior row of rank 0
    is_sep[k] = p->kf_ntouch[k] >= 2;
  }
  const int rc = finish_plan(p, link_dom, is_sep);
  if (rc)
  {
    delete p;
    return rc;
  }
  *out = p;
  return SAGE_OK;
}

// Domains of ONE assembled system (host threads instead of ranks): keyframe k belongs to domain k * ndomains / K; of
// every link that crosses a domain boundary the newer keyframe becomes a separator (the first 3 keyframes of every
// domain in a temporal window; the far end of a loop closure), so no link joins the interiors of two domains.
extern "C" int sage_shard_plan_create_domains(int K, int nlinks, const int32_t *links, int B, int domain, int ndomains,
                                              SageShardPlan **out)
{
  if (!out || K < 1 || B < 1 || nlinks < 0 || (nlinks > 0 && !links) || ndomains < 1 || domain < 0 ||
      domain >= ndomains)
    return SAGE_E_INVALID;
  SageShardPlan *p = new_plan(K, nlinks, links, B, domain, ndomains);
  if (!p)
    return SAGE_E_INVALID;
  p->assembled = true;
  auto dom = [&](int k) { return std::min(ndomains - 1, (int)((long long)k * ndomains / K)); };
  std::vector<char> is_sep(K, 0);
  // long-range links first (loop closures: keyframes further apart than any temporal back-link): their newer end
  // becomes a separator whatever the domains are, so that no envelope row has to span the window
  int span = 0;
  {
    std::vector<int> d(nlinks);
    for (int l = 0; l < nlinks; ++l)
      d[l] = p->links[l].second - p->links[l].first;
    std::vector<int> sorted(d);
    std::sort(sorted.begin(), sorted.end());
    span = nlinks ? std::max(8, 2 * sorted[(size_t)(0.9 * (nlinks - 1))]) : 8; // twice the 90th-percentile link length
    for (int l = 0; l < nlinks; ++l)
      if (d[l] > span && !is_sep[p->links[l].first] && !is_sep[p->links[l].second])
        is_sep[p->links[l].second] = 1;
  }
  for (int l = 0; l < nlinks; ++l)
  {
    const int a = p->links[l].first, b = p->links[l].second;
    if (dom(a) != dom(b) && !is_sep[a] && !is_sep[b])
      is_sep[b] = 1;
  }
  p->kf_owner.assign(K, 0);
  p->kf_ntouch.assign(K, 1);
  for (int k = 0; k < K; ++k)
    p->kf_owner[k] = is_sep[k] ? 0 : dom(k);
  std::vector<int> link_dom(nlinks);
  for (int l = 0; l < nlinks; ++l)
  {
    const int a = p->links[l].first, b = p->links[l].second;
    link_dom[l] = !is_sep[a] ? dom(a) : (!is_sep[b] ? dom(b) : 0); // separator-separator links: domain 0
  }
  const int rc = finish_plan(p, link_dom, is_sep);
  if (rc)
  {
    delete p;
    return rc;
  }
  *out = p;
  return SAGE_OK;
}

extern "C" void sage_shard_plan_destroy(SageShardPlan *p) { delete p; }
extern "C" size_t sage_shard_sep_count(const SageShardPlan *p) { return p ? p->sep_doubles : 0; }
extern "C" int sage_shard_num_separators(const SageShardPlan *p) { return p ? (int)p->sep_all.size() : 0; }
extern "C" int sage_shard_num_interior(const SageShardPlan *p) { return p ? (int)p->interior.size() : 0; }
extern "C" int sage_shard_keyframe_owner(const SageShardPlan *p, int kf)
{
  return (p && kf >= 0 && kf < p->K) ? p->kf_owner[kf] : -1;
}
extern "C" int sage_shard_keyframe_is_local(const SageShardPlan *p, int kf)
{
  if (!p || kf < 0 || kf >= p->K)
    return 0;
  if (p->int_pos[kf] >= 0)
    return 1;
  const int s = p->sep_index[kf];
  return s >= 0 && std::find(p->sep_local.begin(), p->sep_local.end(), s) != p->sep_local.end();
}

// what is specific to a rank's contribution  A^(r) = H^(r) + P^(r) + damp * diag(...)  (elements: damped_system.h): a
// keyframe's prior is added by its owner only; a separator's diagonal block and right-hand side come from every rank that
// touches it (rank mode: its packed buffer only holds its own edge sums) or, when the buffer is the complete assembled
// system, from domain 0 alone
namespace
{
struct LocalSystem
{
  const SageShardPlan &p;
  bool owns_prior(int k) const { return p.kf_owner[k] == p.rank; }
  bool contributes(bool interior) const { return interior || !p.assembled || p.rank == 0; }
};
} // namespace

// the local system's storage (interior rows first, the rank's separators last; no A ranges) as the block solver sees it
static sage::BlockEnvelope local_envelope(const SageShardPlan &p)
{
  sage::BlockEnvelope env;
  env.K = p.nloc;
  env.Bp = p.Bp;
  env.row_first = p.row_first.data();
  env.row_off = p.row_off.data();
  return env;
}

extern "C" int sage_shard_eliminate(SageShardPlan *p, const double *packed_local, double damp, const double *diag_add,
                                    const double *g_add, double *sep_out)
{
  if (!p || !packed_local || !sep_out)
    return SAGE_E_INVALID;
  const int B = p->B, BB = B * B, K = p->K;
  const LocalSystem S{*p};
  const double *diag = packed_local, *lnk = diag + (size_t)K * BB, *g = lnk + (size_t)p->nlinks * BB;
  static const bool dbg = sage::env_flag("SAGE_DEBUG_TIMING");
  auto tnow = [] { return std::chrono::steady_clock::now(); };
  const auto t0 = tnow();
  const int nI = (int)p->interior.size(), nS = (int)p->sep_local.size();
  std::fill(sep_out, sep_out + p->sep_doubles, 0.0);
  double *sep_rhs = sep_out + (size_t)p->n_pair_blocks * BB;
  // tail: this rank's error / inlier totals at the linearisation point ride along
  const double *tail = packed_local + (size_t)(K + p->nlinks) * BB + (size_t)K * B;
  double *sep_tail = sep_rhs + p->sep_all.size() * (size_t)B;
  for (int i = 0; i < 4; ++i)
    sep_tail[i] = (!p->assembled || p->rank == 0) ? tail[i] : 0.0;
  // local separator position of a keyframe (or -1)
  std::vector<int> spos(K, -1);
  for (int i = 0; i < nS; ++i)
    spos[p->sep_all[p->sep_local[i]]] = i;
  const int Bp = p->Bp;
  std::fill(p->T.begin(), p->T.end(), 0.0);
  std::fill(p->yv.begin(), p->yv.end(), 0.0);
  const sage::BlockEnvelope env = local_envelope(*p);
  auto blk = [&](int i, int j) { return env.block(p->T.data(), i, j); };
  auto lpos = [&](int k) { return p->int_pos[k] >= 0 ? p->int_pos[k] : (spos[k] >= 0 ? nI + spos[k] : -1); };
  for (int q = 0; q < p->nloc; ++q)
  {
    const int k = q < nI ? p->interior[q] : p->sep_all[p->sep_local[q - nI]];
    const bool contributes = S.contributes(q < nI), prior = S.owns_prior(k);
    double *D = blk(q, q);
    for (int r = 0; r < Bp; ++r)
      for (int c = 0; c < Bp; ++c)
      {
        double v = sage::damped_pad_elem(r, c, damp);
        if (r < B && c < B)
          v = contributes ? sage::damped_diag_elem(diag + (size_t)k * BB, B, r, c,
                                                   (diag_add && prior) ? diag_add[(size_t)k * B + r] : 0.0, damp)
                          : 0.0;
        D[sage::stored_slot(r, c, Bp)] = v;
      }
    if (contributes)
      for (int r = 0; r < B; ++r)
        p->yv[(size_t)q * Bp + r] =
            sage::damped_rhs_elem(g[(size_t)k * B + r], (g_add && prior) ? g_add[(size_t)k * B + r] : 0.0);
  }
  for (int l : p->local_links)
  {
    const int a = p->links[l].first, b = p->links[l].second;
    const int qa = lpos(a), qb = lpos(b);
    if (qa < 0 || qb < 0)
      return SAGE_E_STATE;
    const int qi = std::max(qa, qb), qj = std::min(qa, qb);
    double *D = blk(qi, qj);
    const bool row_is_a = qi == qa;
    for (int r = 0; r < B; ++r)
      for (int c = 0; c < B; ++c)
        D[sage::stored_slot(r, c, Bp)] += lnk[(size_t)l * BB + sage::link_elem(row_is_a, r, c, B)];
  }
  const auto t1 = tnow();
  const int rcf = sage::block_chol_partial(env, p->T.data(), p->X.data(), p->yv.data(), nI);
  if (rcf != 0)
    return SAGE_E_NOT_PSD;
  p->have_factor = true;
  // Schur complement blocks and right-hand side of this rank's separators -> separator buffer
  for (int i = 0; i < nS; ++i)
  {
    for (int j = 0; j <= i; ++j)
    {
      if (nI + j < p->row_first[nI + i])
        continue; // outside the envelope: structurally zero
      const auto it = p->pair_block.find({p->sep_local[j], p->sep_local[i]});
      if (it == p->pair_block.end())
        continue; // (inside the envelope but coupled by nothing: zero)
      const double *src = blk(nI + i, nI + j); // [cc][rr] = C[(s_i, rr), (s_j, cc)], valid for rr >= cc when i == j
      double *dst = sep_out + (size_t)it->second * BB; // rows s_j, cols s_i
      for (int r = 0; r < B; ++r)
        for (int c = 0; c < B; ++c)
          dst[r * B + c] = (i != j || c >= r) ? src[r * Bp + c] : src[c * Bp + r];
    }
    for (int r = 0; r < B; ++r)
      sep_rhs[(size_t)p->sep_local[i] * B + r] = p->yv[(size_t)(nI + i) * Bp + r];
  }
  if (dbg)
  {
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[sage shard eliminate] fixed-block: build %.3f partial factorisation %.3f scatter %.3f ms (%d interior, %d separators)\n",
            ms(t0, t1), ms(t1, tnow()), 0.0, nI, nS);
  }
  return SAGE_OK;
}

extern "C" int sage_shard_solve(SageShardPlan *p, const double *sep_reduced, double *delta)
{
  if (!p || !sep_reduced || !delta || !p->have_factor)
    return SAGE_E_STATE;
  const int B = p->B;
  const int nSa = (int)p->sep_all.size(), NSa = nSa * B;
  std::vector<double> dS(NSa, 0.0);
  if (NSa > 0)
  {
    // the reduced buffer IS a packed block system over the separator keyframes (diag | coupled pairs | rhs): the
    // fixed-block AVX-512 factorisation of the window solve takes it as it is (no damping, no priors: both are inside)
    const int rc = sage_block_solve(sep_reduced, nSa, (int)p->sep_pairs.size() / 2, p->sep_pairs.data(), B, 0.0, nullptr,
                                    nullptr, dS.data());
    if (rc)
      return rc;
  }
  const int Bp = p->Bp, nI = (int)p->interior.size(), nS = (int)p->sep_local.size();
  for (int s = 0; s < nS; ++s)
  {
    for (int r = 0; r < B; ++r)
      p->yv[(size_t)(nI + s) * Bp + r] = dS[(size_t)p->sep_local[s] * B + r];
    for (int r = B; r < Bp; ++r)
      p->yv[(size_t)(nI + s) * Bp + r] = 0.0;
  }
  const sage::BlockEnvelope env = local_envelope(*p);
  if (sage::block_chol_partial_back(env, p->T.data(), p->X.data(), p->yv.data(), nI) != 0)
    return SAGE_E_STATE;
  for (int i = 0; i < nI; ++i)
    for (int r = 0; r < B; ++r)
      delta[(size_t)p->interior[i] * B + r] = p->yv[(size_t)i * Bp + r];
  for (int s = 0; s < nS; ++s)
    for (int r = 0; r < B; ++r)
      delta[(size_t)p->sep_all[p->sep_local[s]] * B + r] = dS[(size_t)p->sep_local[s] * B + r];
  return SAGE_OK;
}

// ------------------------------------------------------------------------------------------------
// One process, several host threads: the damped solve of an ASSEMBLED window system by domain decomposition.
// Same contract as sage_block_solve; meant for windows the banded factorisation handles badly: long windows (the
// domains are eliminated in parallel) and loop closures (their far ends become separators instead of envelope rows
// that span the whole window).
// ------------------------------------------------------------------------------------------------
#include <thread>

extern "C" int sage_block_solve_domains(const double *packed, int K, int nlinks, const int32_t *links, int B,
                                        double damp, const double *diag_add, const double *g_add, int ndomains,
                                        double *delta)
{
  if (!packed || !delta || K < 1 || B < 1 || ndomains < 1)
    return SAGE_E_INVALID;
  ndomains = std::min(ndomains, std::max(1, K / 4));
  std::vector<SageShardPlan *> plans(ndomains, nullptr);
  int rc = SAGE_OK;
  for (int d = 0; d < ndomains && !rc; ++d)
    rc = sage_shard_plan_create_domains(K, nlinks, links, B, d, ndomains, &plans[d]);
  std::vector<std::vector<double>> sep(ndomains);
  std::vector<int> rcs(ndomains, 0);
  if (!rc)
  {
    const size_t n = sage_shard_sep_count(plans[0]);
    std::vector<std::thread> th;
    for (int d = 0; d < ndomains; ++d)
    {
      sep[d].assign(n, 0.0);
      auto job = [&, d] { rcs[d] = sage_shard_eliminate(plans[d], packed, damp, diag_add, g_add, sep[d].data()); };
      if (d + 1 < ndomains)
        th.emplace_back(job);
      else
        job();
    }
    for (auto &t : th)
      t.join();
    for (int d = 0; d < ndomains; ++d)
      if (rcs[d])
        rc = rcs[d];
    if (!rc)
    {
      for (int d = 1; d < ndomains; ++d)
        for (size_t i = 0; i < n; ++i)
          sep[0][i] += sep[d][i];
      std::fill(delta, delta + (size_t)K * B, 0.0);
      th.clear();
      // every domain solves into a buffer of its own: a separator keyframe next to two domains is written by both (the same
      // values, but two threads storing to one address is still a data race -- found with ThreadSanitizer); merged below
      std::vector<std::vector<double>> dd((size_t)ndomains, std::vector<double>((size_t)K * B, 0.0));
      for (int d = 0; d < ndomains; ++d)
      {
        auto job = [&, d] { rcs[d] = sage_shard_solve(plans[d], sep[0].data(), dd[d].data()); };
        if (d + 1 < ndomains)
          th.emplace_back(job);
        else
          job();
      }
      for (auto &t : th)
        t.join();
      for (int d = 0; d < ndomains; ++d)
        if (rcs[d])
          rc = rcs[d];
      // (an interior keyframe has one owner, a separator's rows are identical in every domain that holds it)
      for (int d = 0; d < ndomains; ++d)
        for (size_t i = 0; i < (size_t)K * B; ++i)
          if (dd[d][i] != 0.0)
            delta[i] = dd[d][i];
    }
  }
  for (SageShardPlan *p : plans)
    sage_shard_plan_destroy(p);
  return rc;
}
