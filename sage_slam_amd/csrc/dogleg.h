// dogleg.h -- Powell's dogleg on the window's system, the host side (no HIP): what a trial point is in terms of the six dot
// products, and the layout the product kernels (window_dogleg.hip) and their host plan (dogleg_host.cpp) share.
//
// Every trial point of an iteration is  delta = a g + b n  (g: the right-hand side, n = A^-1 g).  With
//   dots = { g.g, g.n, n.n, g.Ag, g.An, n.An }
// its squared norm and the decrease of the engine's error model E(x (+) delta) ~ E(x) - 2 g.delta + delta.A delta follow
// without touching a vector again.
#pragma once
#include <cstdint>

#include "damped_system.h" // SAGE_HD

namespace sage
{
namespace dogleg
{

enum : int { kGG = 0, kGN = 1, kNN = 2, kGAG = 3, kGAN = 4, kNAN = 5, kDots = 6 };

inline double step_norm2(const double *d, double a, double b)
{
  return a * a * d[kGG] + 2.0 * a * b * d[kGN] + b * b * d[kNN];
}

// 2 g.delta - delta.A delta
inline double model_decrease(const double *d, double a, double b)
{
  return 2.0 * (a * d[kGG] + b * d[kGN]) - (a * a * d[kGAG] + 2.0 * a * b * d[kGAN] + b * b * d[kNAN]);
}

// the product kernels' partial sums: one slot of [2][B] doubles (the block times g, times n) per incidence entry
// (sage_dogleg_incidence) -- a diagonal block's at its keyframe, a link's direct and transposed products behind them
SAGE_HD inline int partial_slot(int K, int block, int transposed) { return block < K ? block : K + 2 * (block - K) + transposed; }
SAGE_HD inline int partial_slots(int K, int nlinks) { return K + 2 * nlinks; }

// the pinned record the products land in: the dots, |An - g|^2, and the ticket (the epoch of the call that wrote them)
struct HostRecord
{
  double dots[kDots];
  double resid2;
  double ticket;
};

} // namespace dogleg
} // namespace sage
