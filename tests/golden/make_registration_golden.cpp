// Golden results of teaser::RobustRegistrationSolver::solve(src, dst, noise_bounds) in the reference's shipped configuration
// (inlier_selection_mode none, chain TIMs for the rotation, GNC-TLS, estimate_scaling) -- the solve behind
// CameraTracker::FeatureMatchingGeo and MatchGeometryFactor -- produced by the reference's OWN solver: this file is compiled
// together with thirdparty/TEASER-plusplus/teaser/src/registration.cc against the TEASER++ headers and the vendored Eigen of
// the reference's thirdparty tree (build container only; tests/golden/make_registration_golden.py drives it):
//   g++ -O2 -DNDEBUG -std=c++14 -I<thirdparty>/TEASER-plusplus/teaser/include -I<thirdparty>/eigen \
//       tests/golden/make_registration_golden.cpp <thirdparty>/TEASER-plusplus/teaser/src/registration.cc -o regen
//   regen < problem.txt > result.txt
// stdin:  N noise_bound cbar2 max_iterations cost_threshold gnc_factor, then N rows "sx sy sz dx dy dz nb" (fp32 values;
//         they are read as float and widened to double, as the reference widens its fp32 tensors)
// stdout: valid, scale, R (row-major), t, rotation_cost, scale_inliers (the count of the pairs' mask), rotation_mask,
//         inliers (getTranslationInliers), all floating-point values as %.17g
// registration.cc refers to the max-clique solver, which the mode `none` never calls: its one undefined symbol is defined
// here as a stub that aborts.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "teaser/graph.h"
#include "teaser/registration.h"

std::vector<int> teaser::MaxCliqueSolver::findMaxClique(teaser::Graph)
{
  std::fprintf(stderr, "findMaxClique called: the generator runs inlier_selection_mode none only\n");
  std::abort();
}

int main()
{
  int N = 0, max_iterations = 0;
  double noise_bound = 0, cbar2 = 0, cost_threshold = 0, gnc_factor = 0;
  if (std::scanf("%d %lf %lf %d %lf %lf", &N, &noise_bound, &cbar2, &max_iterations, &cost_threshold, &gnc_factor) != 6 || N < 2)
    return 2;
  Eigen::Matrix<double, 3, Eigen::Dynamic> src(3, N), dst(3, N);
  Eigen::Matrix<double, 1, Eigen::Dynamic> nb(1, N);
  for (int i = 0; i < N; ++i)
  {
    float v[7];
    for (int c = 0; c < 7; ++c)
      if (std::scanf("%f", &v[c]) != 1)
        return 2;
    for (int c = 0; c < 3; ++c)
    {
      src(c, i) = (double)v[c];
      dst(c, i) = (double)v[3 + c];
    }
    nb(0, i) = (double)v[6];
  }
  teaser::RobustRegistrationSolver::Params params;
  params.noise_bound = noise_bound;
  params.cbar2 = cbar2;
  params.estimate_scaling = true;
  params.rotation_estimation_algorithm = teaser::RobustRegistrationSolver::ROTATION_ESTIMATION_ALGORITHM::GNC_TLS;
  params.rotation_gnc_factor = gnc_factor;
  params.rotation_max_iterations = (size_t)max_iterations;
  params.rotation_cost_threshold = cost_threshold;
  params.rotation_tim_graph = teaser::RobustRegistrationSolver::INLIER_GRAPH_FORMULATION::CHAIN;
  params.inlier_selection_mode = teaser::RobustRegistrationSolver::INLIER_SELECTION_MODE::NONE;
  teaser::RobustRegistrationSolver solver(params);
  solver.solve(src, dst, nb);
  const teaser::RegistrationSolution sol = solver.getSolution();
  std::printf("valid %d\nscale %.17g\nR", sol.valid ? 1 : 0, sol.scale);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      std::printf(" %.17g", sol.rotation(r, c));
  std::printf("\nt %.17g %.17g %.17g\n", sol.translation(0), sol.translation(1), sol.translation(2));
  std::printf("rotation_cost %.17g\n", solver.getGNCRotationCostAtTermination());
  const auto scale_mask = solver.getScaleInliersMask();
  long n_scale = 0;
  for (long i = 0; i < scale_mask.cols(); ++i)
    n_scale += scale_mask(0, i) ? 1 : 0;
  std::printf("scale_inliers %ld\n", n_scale);
  const auto rot_mask = solver.getRotationInliersMask();
  std::printf("rotation_mask");
  for (long i = 0; i < rot_mask.cols(); ++i)
    std::printf(" %d", rot_mask(0, i) ? 1 : 0);
  const std::vector<int> inl = solver.getTranslationInliers();
  std::printf("\ninliers");
  for (int i : inl)
    std::printf(" %d", i);
  std::printf("\n");
  return 0;
}
