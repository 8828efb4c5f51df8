// marginal_check.cpp -- host-only driver of sage_schur_marginal (sage_slam_amd/csrc/marginal_host.cpp), meant to be built
// with -fsanitize=address,undefined and run on the CPU (tests/test_marginal_host.py does both).  Links marginal_host.cpp
// alone: no HIP, no engine library.  Two cases on random SPD systems, n = 3 * 23 and 4 * 39:
//   1. the marginal against a Gauss-Jordan elimination in long double, symmetry of Lambda, a non-positive pivot's status
//      with untouched outputs, identity drop rows as a no-op;
//   2. Schur of Schur: dropping block 0 and then block 1 of the result against dropping both at once.
// Bound: 64 n 2^-53 cond(A_dd) in relative Frobenius norm, cond bounded by the spectrum the systems are built with (1e4).
// Exit status 0: every check passed; otherwise the number of failed checks (each one printed).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

#include "sage_ba.h"

typedef std::vector<double> Vec;

static int g_failed = 0;
static void check(bool ok, const char *what, double got = 0.0, double bar = 0.0)
{
  if (!ok)
  {
    ++g_failed;
    std::printf("FAILED %s (%.3e against %.3e)\n", what, got, bar);
  }
}

// A = sum_i lambda_i v_i v_i^T over a random orthonormal basis (Gram-Schmidt), lambda log-spaced in [1 / cond, 1]
static Vec random_spd(int n, double cond, std::mt19937_64 &rng)
{
  std::normal_distribution<double> nd;
  std::vector<Vec> q(n, Vec(n));
  for (int i = 0; i < n; ++i)
  {
    for (double &v : q[i])
      v = nd(rng);
    for (int pass = 0; pass < 2; ++pass)
      for (int j = 0; j < i; ++j)
      {
        const double d = std::inner_product(q[i].begin(), q[i].end(), q[j].begin(), 0.0);
        for (int k = 0; k < n; ++k)
          q[i][k] -= d * q[j][k];
      }
    const double nrm = std::sqrt(std::inner_product(q[i].begin(), q[i].end(), q[i].begin(), 0.0));
    for (double &v : q[i])
      v /= nrm;
  }
  Vec A((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i)
  {
    const double lam = std::pow(cond, -(double)i / (n - 1));
    for (int r = 0; r < n; ++r)
      for (int c = 0; c < n; ++c)
        A[(size_t)r * n + c] += lam * q[i][r] * q[i][c];
  }
  return A;
}

// the same marginal by Gauss-Jordan elimination of the drop rows in long double (pivots on the diagonal: SPD)
static void reference_marginal(const Vec &A, const Vec &g, double e, int n, const std::vector<int32_t> &drop, Vec &Lam, Vec &eta, double &c)
{
  std::vector<long double> M((size_t)n * n), v(g.begin(), g.end());
  for (int r = 0; r < n; ++r)
    for (int col = 0; col < n; ++col)
      M[(size_t)r * n + col] = 0.5L * ((long double)A[(size_t)r * n + col] + (long double)A[(size_t)col * n + r]);
  long double ee = e;
  std::vector<char> gone(n, 0);
  for (int d : drop)
  {
    const long double piv = M[(size_t)d * n + d];
    ee -= v[d] * v[d] / piv;
    for (int r = 0; r < n; ++r)
    {
      if (r == d || gone[r])
        continue;
      const long double f = M[(size_t)r * n + d] / piv;
      for (int col = 0; col < n; ++col)
        if (!gone[col])
          M[(size_t)r * n + col] -= f * M[(size_t)d * n + col];
      v[r] -= f * v[d];
    }
    gone[d] = 1;
  }
  std::vector<int> keep;
  for (int i = 0; i < n; ++i)
    if (!gone[i])
      keep.push_back(i);
  const int nk = (int)keep.size();
  Lam.assign((size_t)nk * nk, 0.0);
  eta.assign(nk, 0.0);
  for (int i = 0; i < nk; ++i)
  {
    eta[i] = (double)v[keep[i]];
    for (int j = 0; j < nk; ++j)
      Lam[(size_t)i * nk + j] = (double)(0.5L * (M[(size_t)keep[i] * n + keep[j]] + M[(size_t)keep[j] * n + keep[i]]));
  }
  c = (double)ee;
}

static double rel(const Vec &a, const Vec &b)
{
  double num = 0.0, den = 0.0;
  for (size_t i = 0; i < a.size(); ++i)
  {
    num += (a[i] - b[i]) * (a[i] - b[i]);
    den += b[i] * b[i];
  }
  return std::sqrt(num / (den > 0.0 ? den : 1.0));
}

static std::vector<int32_t> block_rows(std::initializer_list<int> blocks, int B)
{
  std::vector<int32_t> rows;
  for (int b : blocks)
    for (int r = 0; r < B; ++r)
      rows.push_back(b * B + r);
  return rows;
}

static void run(int nb, int B, std::mt19937_64 &rng)
{
  const int n = nb * B;
  const double cond = 1.0e4; // of A; cond(A_dd) <= cond(A) (a principal sub-matrix' spectrum lies inside the matrix')
  const double bar = 64.0 * n * std::ldexp(1.0, -53) * cond;
  const Vec A = random_spd(n, cond, rng);
  Vec g(n);
  std::normal_distribution<double> nd;
  for (double &v : g)
    v = nd(rng);
  const double e = 1.0e5;
  // ---- case 1
  for (int ndrop = 1; ndrop <= 2; ++ndrop)
  {
    const std::vector<int32_t> drop = ndrop == 1 ? block_rows({1}, B) : block_rows({0, 2}, B);
    const int nk = n - (int)drop.size();
    Vec Lam((size_t)nk * nk), eta(nk), LamR, etaR;
    double c = 0.0, cR = 0.0;
    check(sage_schur_marginal(A.data(), g.data(), e, n, drop.data(), (int)drop.size(), Lam.data(), eta.data(), &c) == SAGE_OK, "status");
    reference_marginal(A, g, e, n, drop, LamR, etaR, cR);
    check(rel(Lam, LamR) <= bar, "Lambda", rel(Lam, LamR), bar);
    check(rel(eta, etaR) <= bar, "eta", rel(eta, etaR), bar);
    check(std::fabs(c - cR) <= bar * std::fabs(cR), "c", std::fabs(c - cR), bar * std::fabs(cR));
    bool symmetric = true;
    for (int i = 0; i < nk; ++i)
      for (int j = 0; j < nk; ++j)
        symmetric = symmetric && Lam[(size_t)i * nk + j] == Lam[(size_t)j * nk + i];
    check(symmetric, "Lambda is exactly symmetric");
  }
  {
    // a non-positive pivot: the block solve's status, outputs untouched
    Vec Abad = A;
    Abad[(size_t)(B + 3) * n + B + 3] = -1.0;
    const std::vector<int32_t> drop = block_rows({1}, B);
    const int nk = n - B;
    Vec Lam((size_t)nk * nk, 7.0), eta(nk, 7.0);
    double c = 7.0;
    check(sage_schur_marginal(Abad.data(), g.data(), e, n, drop.data(), B, Lam.data(), eta.data(), &c) == SAGE_E_NOT_PSD, "non-positive pivot");
    bool untouched = c == 7.0;
    for (double v : Lam)
      untouched = untouched && v == 7.0;
    for (double v : eta)
      untouched = untouched && v == 7.0;
    check(untouched, "non-positive pivot writes nothing");
  }
  {
    // identity drop rows (held variables): rows 0 .. 5 of block 1 become rows of the identity with a zero gradient, and
    // dropping block 1 then equals dropping only its other rows from the system without them
    Vec Ah = A, gh = g;
    for (int r = B; r < B + 6; ++r)
    {
      for (int col = 0; col < n; ++col)
        Ah[(size_t)r * n + col] = Ah[(size_t)col * n + r] = 0.0;
      Ah[(size_t)r * n + r] = 1.0;
      gh[r] = 0.0;
    }
    const int n2 = n - 6, nk = n - B;
    Vec As((size_t)n2 * n2), gs(n2);
    auto small = [B](int r) { return r < B ? r : r - 6; };
    for (int r = 0; r < n; ++r)
    {
      if (r >= B && r < B + 6)
        continue;
      gs[small(r)] = gh[r];
      for (int col = 0; col < n; ++col)
        if (!(col >= B && col < B + 6))
          As[(size_t)small(r) * n2 + small(col)] = Ah[(size_t)r * n + col];
    }
    std::vector<int32_t> drop_s;
    for (int r = B; r < 2 * B - 6; ++r)
      drop_s.push_back(r);
    const std::vector<int32_t> drop = block_rows({1}, B);
    Vec L1((size_t)nk * nk), e1(nk), L2((size_t)nk * nk), e2(nk);
    double c1 = 0.0, c2 = 0.0;
    check(sage_schur_marginal(Ah.data(), gh.data(), e, n, drop.data(), B, L1.data(), e1.data(), &c1) == SAGE_OK, "status (held)");
    check(sage_schur_marginal(As.data(), gs.data(), e, n2, drop_s.data(), (int)drop_s.size(), L2.data(), e2.data(), &c2) == SAGE_OK, "status (small)");
    check(L1 == L2 && e1 == e2 && c1 == c2, "identity drop rows eliminate to nothing");
  }
  // ---- case 2: Schur of Schur
  {
    const std::vector<int32_t> d0 = block_rows({0}, B), d01 = block_rows({0, 1}, B);
    const int n1 = n - B, n2 = n - 2 * B;
    Vec La((size_t)n1 * n1), ea(n1), Lb((size_t)n2 * n2), eb(n2), Lc((size_t)n2 * n2), ec(n2);
    double ca = 0.0, cb = 0.0, cc = 0.0;
    check(sage_schur_marginal(A.data(), g.data(), e, n, d0.data(), B, La.data(), ea.data(), &ca) == SAGE_OK, "status (first)");
    check(sage_schur_marginal(La.data(), ea.data(), ca, n1, d0.data(), B, Lb.data(), eb.data(), &cb) == SAGE_OK, "status (second)");
    check(sage_schur_marginal(A.data(), g.data(), e, n, d01.data(), 2 * B, Lc.data(), ec.data(), &cc) == SAGE_OK, "status (both)");
    check(rel(Lb, Lc) <= bar, "Schur of Schur: Lambda", rel(Lb, Lc), bar);
    check(rel(eb, ec) <= bar, "Schur of Schur: eta", rel(eb, ec), bar);
    check(std::fabs(cb - cc) <= bar * std::fabs(cc), "Schur of Schur: c", std::fabs(cb - cc), bar * std::fabs(cc));
  }
}

int main()
{
  std::mt19937_64 rng(7);
  run(3, 23, rng);
  run(4, 39, rng);
  std::printf("%s (%d failed)\n", g_failed ? "marginal_check FAILED" : "marginal_check ok", g_failed);
  return g_failed;
}
