// convex_hull.cpp -- sage_convex_hull_area: the host half of sage_track_overlap (overlap.hip), and the whole of the
// reference's way to the same numbers (boost::geometry::convex_hull + area over every point, camera_tracker.cpp:130-152).
// Stateless, no device, nothing but the public header: compiles on its own for a sanitizer run.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "sage_ba.h"

namespace
{
typedef std::pair<double, double> Pt; // (x, y): pair's operator< is the lexicographic order the chain is built in

// > 0: c lies to the left of a -> b.  Differences of fp32-valued doubles are exact, their products too
inline double turn(const Pt &a, const Pt &b, const Pt &c)
{
  return (b.first - a.first) * (c.second - a.second) - (b.second - a.second) * (c.first - a.first);
}
} // namespace

// Andrew's monotone chain over the sorted, de-duplicated points; collinear boundary points are popped (strict turns only),
// so the vertex count is the number of corners.  The shoelace sum runs over the chain in its own order: the caller's order
// never reaches the result.
extern "C" int sage_convex_hull_area(const float *xy, int n, double *area, int *n_vertices)
{
  if (!area || n < 0 || (n > 0 && !xy))
    return SAGE_E_INVALID;
  *area = 0.0;
  if (n_vertices)
    *n_vertices = 0;
  std::vector<Pt> p;
  p.reserve((size_t)n);
  for (int i = 0; i < n; ++i)
    if (std::isfinite(xy[2 * i]) && std::isfinite(xy[2 * i + 1])) // (a NaN would also break the sort's ordering)
      p.emplace_back((double)xy[2 * i], (double)xy[2 * i + 1]);
  std::sort(p.begin(), p.end());
  p.erase(std::unique(p.begin(), p.end()), p.end());
  const size_t m = p.size();
  if (m < 3)
    return SAGE_OK;
  std::vector<Pt> h(2 * m);
  size_t k = 0;
  for (size_t i = 0; i < m; ++i) // lower chain
  {
    while (k >= 2 && turn(h[k - 2], h[k - 1], p[i]) <= 0.0)
      --k;
    h[k++] = p[i];
  }
  const size_t lower = k + 1;
  for (size_t i = m - 1; i-- > 0;) // upper chain
  {
    while (k >= lower && turn(h[k - 2], h[k - 1], p[i]) <= 0.0)
      --k;
    h[k++] = p[i];
  }
  --k; // (the first point closes the chain)
  if (k < 3)
    return SAGE_OK; // collinear
  double twice = 0.0;
  for (size_t i = 0; i < k; ++i) // shoelace about the first corner: small terms for a hull far from the origin
  {
    const Pt &a = h[i], &b = h[(i + 1) % k];
    twice += (a.first - h[0].first) * (b.second - h[0].second) - (b.first - h[0].first) * (a.second - h[0].second);
  }
  *area = 0.5 * twice;
  if (n_vertices)
    *n_vertices = (int)k;
  return SAGE_OK;
}
