// sage_gtsam_prepass.h -- gtsam side of SURVEY s8 f2: serve PhotometricFactor / GeometricFactor ::linearize / ::error
// (core/gtsam/photometric_factor.cpp:72-219, geometric_factor.cpp:41-233) from ONE batched window evaluation per
// gtsam::Values instead of one kernel sequence + NearestPsd per factor.
//
// NOT LINKED AGAINST gtsam IN THIS IMAGE: gtsam needs Boost, which the build container lacks; the header is
// put through a compiler with the real Eigen / Sophus and syntax-check stand-ins for gtsam / boost
// (integration/compile_check, tests/test_adapter_compiles.py).  Everything below the
// gtsam types -- value comparison, batched linearize / error pass, device-to-host copy of the per-edge results,
// NearestPsd (as written or Higham), the cut into the reference's G11..Gnn / g1..gn order -- is engine code behind the
// C ABI (sage_window_prepass / sage_window_factor / sage_window_factor_error and, for the window's keypoint and graph terms,
// sage_window_keypoint_factor / sage_window_graph_factor: include/sage_ba.h) and is tested on the GPU against the oracle
// (tests/test_gpu_factor_cache.py, tests/test_gpu_term_factor_cache.py); this header is the type conversion that remains.
//
// Use: Mapper owns one SageWindowCache per active window (keyframes + links registered as in INTEGRATION.md s3) and
// hands it to the factors it creates; the two factor classes replace the bodies of linearize() / error() as shown.
#pragma once
#include <gtsam/linear/HessianFactor.h>
#include <gtsam/nonlinear/Values.h>
#include <sophus/se3.hpp>

#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "sage_ba.h"

namespace df
{

class SageWindowCache
{
public:
  struct Keys
  {
    gtsam::Key pose, code, scale;
  };

  // keys[k]: the gtsam keys of window keyframe k (the order of sage_window_add_keyframe)
  // device_psd (opt-in, psd_mode 1 only): the eager projection runs on the device (sage_window_prepare_factors_device)
  // instead of on host threads; any other psd_mode ignores the switch
  SageWindowCache(SageWindow *win, std::vector<Keys> keys, int code_size, int psd_mode /* 2 = NearestPsd as written */,
                  bool device_psd = false)
      : win_(win), keys_(std::move(keys)), CS_(code_size), psd_mode_(psd_mode), device_psd_(device_psd && psd_mode == 1),
        pose_(keys_.size() * 12), code_(keys_.size() * code_size), scale_(keys_.size())
  {
    for (size_t k = 0; k < keys_.size(); ++k) // start from the variables the keyframes were added with
      sage_window_get_keyframe(win_, (int)k, &pose_[k * 12], &code_[k * CS_], &scale_[k]);
  }

  // SAGE_RELIN_STALE (opt-in; SAGE_RELIN_ALL is the window's default): a recomputing Prepare with jacobians evaluates only
  // the dense edges that read a key whose value differs from the last linearisation's, and copies only their rows -- what an
  // unmodified ISAM2 (cacheLinearizedFactors, relinearizeSkip 1) asks for after it has moved a few keys; the served factors
  // are the same bytes either way.  Call it once, after the window is finalized; sharded windows refuse the mode
  bool SetRelinearization(int mode)
  {
    std::lock_guard<std::mutex> lock(mutex_);
    return sage_window_set_relinearization(win_, mode) == SAGE_OK;
  }

  // Gather the window's variables out of `c` (pose_wk as [R row-major | t], gtsam_traits.h:45-70) and make sure the
  // cache holds their linearisation (jacobians) or errors.  The first factor that sees new Values pays for the whole
  // window; every other factor of the same ISAM2 relinearisation / Dogleg trial is a cache hit.
  // (called with mutex_ held: the prepass and the read of its result must not interleave with another thread's Values)
  bool Prepare(const gtsam::Values &c, bool jacobians)
  {
    for (size_t k = 0; k < keys_.size(); ++k)
    {
      if (!c.exists(keys_[k].pose)) // keyframe marginalised out of this Values: keep the engine's current value
        continue;
      const Sophus::SE3f T = c.at<Sophus::SE3f>(keys_[k].pose);
      const Eigen::Matrix3f R = T.rotationMatrix();
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          pose_[k * 12 + i * 3 + j] = R(i, j);
      for (int i = 0; i < 3; ++i)
        pose_[k * 12 + 9 + i] = T.translation()(i);
      const gtsam::Vector code = c.at<gtsam::Vector>(keys_[k].code);
      for (int i = 0; i < CS_; ++i)
        code_[k * CS_ + i] = (float)code(i);
      scale_[k] = c.at<float>(keys_[k].scale);
    }
    int recomputed = 0;
    Check(sage_window_prepass(win_, pose_.data(), code_.data(), scale_.data(), jacobians ? 1 : 0, &recomputed), "sage_window_prepass");
    // the per-factor NearestPsd (the host cost of linearize(): an SVD of a 45 x 45 / 78 x 78 matrix each) for the whole
    // window at once on the host's cores; Linearize() below then only cuts blocks
    if (recomputed && jacobians && eager_psd_threads_ >= 0)
    {
      // a failed projection is not fatal here: the cache is marked unprepared by the engine and Linearize() projects the
      // factors it is asked for one by one (and reports their errors)
      const int rcp = device_psd_ ? sage_window_prepare_factors_device(win_, nullptr)
                                  : sage_window_prepare_factors(win_, psd_mode_, eager_psd_threads_);
      if (rcp != SAGE_OK)
        fprintf(stderr, "%s: %s (falling back to per-factor projection)\n",
                device_psd_ ? "sage_window_prepare_factors_device" : "sage_window_prepare_factors", sage_error_string(rcp));
    }
    return recomputed != 0;
  }

  // PhotometricFactor::linearize (type 0, keys {p0,p1,c0,s0}) / GeometricFactor::linearize (type 1, keys
  // {p0,p1,c0,c1,s0,s1}); edge = 2 * link + direction as sage_window_get_edge numbers them
  boost::shared_ptr<gtsam::HessianFactor> Linearize(const gtsam::Values &c, int type, int edge,
                                                    const gtsam::FastVector<gtsam::Key> &factor_keys)
  {
    return ServeLinearize(c, factor_keys, sage_factor_block_count(type, CS_), "sage_window_factor",
                          [&](double *G, double *g, double *f, int32_t *dims, int32_t *nkeys)
                          { return sage_window_factor(win_, type, edge, psd_mode_, G, g, f, dims, nkeys); });
  }

  // PhotometricFactor::error / GeometricFactor::error (photometric_factor.cpp:72-101, geometric_factor.cpp:41-64)
  double Error(const gtsam::Values &c, int type, int edge)
  {
    return ServeError(c, "sage_window_factor_error", [&](double *e) { return sage_window_factor_error(win_, type, edge, e); });
  }

  // The window's terms (sage_window_add_keypoint_term / sage_window_add_graph_term; `term` is the id the add call returned)
  // behind the same cache and the same Prepare: family SAGE_TERM_KEYPOINT with kind SAGE_KP_* serves
  // ReprojectionFactor::linearize (keys {p0,p1,c0,s0}), MatchGeometryFactor (keys {p0,p1,c0,c1,s0,s1}) and LoopMGFactor
  // (keys {p0,p1,s0,s1}); family SAGE_TERM_GRAPH with kind SAGE_GRAPH_* serves RelPoseScaleFactor (keys {p0,p1,s0,s1}),
  // RelPoseFactor (keys {p0,p1}) and ScaleFactor (key {s}).  Each is projected on its own matrix, as the reference's
  // linearize() projects its own AtA (match_geometry_factor.cpp:295, reprojection_factor.cpp:245, loop_mg_factor.cpp:90,
  // rel_pose_scale_factor.cpp:132, rel_pose_factor.cpp:110, scale_factor.cpp:68)
  boost::shared_ptr<gtsam::HessianFactor> LinearizeTerm(const gtsam::Values &c, int family, int kind, int term,
                                                        const gtsam::FastVector<gtsam::Key> &factor_keys)
  {
    const bool graph = family == SAGE_TERM_GRAPH;
    return ServeLinearize(c, factor_keys, sage_term_factor_block_count(family, kind, CS_),
                          graph ? "sage_window_graph_factor" : "sage_window_keypoint_factor",
                          [&](double *G, double *g, double *f, int32_t *dims, int32_t *nkeys)
                          { return (graph ? sage_window_graph_factor : sage_window_keypoint_factor)(win_, term, psd_mode_, G, g, f, dims, nkeys); });
  }

  double ErrorTerm(const gtsam::Values &c, int family, int term)
  {
    const bool graph = family == SAGE_TERM_GRAPH;
    return ServeError(c, graph ? "sage_window_graph_factor_error" : "sage_window_keypoint_factor_error",
                      [&](double *e) { return (graph ? sage_window_graph_factor_error : sage_window_keypoint_factor_error)(win_, term, e); });
  }

private:
  static void Check(int rc, const char *name) // the reference's gpuErrchk convention
  {
    if (rc == SAGE_OK)
      return;
    fprintf(stderr, "%s: %s\n", name, sage_error_string(rc));
    exit(rc);
  }

  // one linearize(): the cache at these Values, room for `count` doubles of blocks (a negative count: the status of the
  // block-count call), the engine's read `call` (named `name` in the message), the blocks as a HessianFactor
  template <class Call>
  boost::shared_ptr<gtsam::HessianFactor> ServeLinearize(const gtsam::Values &c, const gtsam::FastVector<gtsam::Key> &factor_keys,
                                                         int count, const char *name, Call call)
  {
    std::lock_guard<std::mutex> lock(mutex_); // factors are called from up to 4 host threads (deepfactors.cpp:1497-1505)
    Prepare(c, true);
    Check(count < 0 ? count : SAGE_OK, "factor block count");
    std::vector<double> G(count), g(14 + 2 * CS_); // (the widest factor)
    int32_t dims[6], nkeys = 0;
    double f = 0.0;
    Check(call(G.data(), g.data(), &f, dims, &nkeys), name);
    return Assemble(factor_keys, G, g, dims, nkeys, f);
  }

  // one error(): the same for the factor's error
  template <class Call>
  double ServeError(const gtsam::Values &c, const char *name, Call call)
  {
    std::lock_guard<std::mutex> lock(mutex_);
    Prepare(c, false);
    double e = 0.0;
    Check(call(&e), name);
    return e;
  }

  // the upper-triangular blocks and g as the engine packs them -> gtsam::HessianFactor(keys, Gs, gs, f)
  static boost::shared_ptr<gtsam::HessianFactor> Assemble(const gtsam::FastVector<gtsam::Key> &factor_keys,
                                                          const std::vector<double> &G, const std::vector<double> &g,
                                                          const int *dims, int nkeys, double f)
  {
    using RowMajor = Eigen::Matrix<double, Eigen::Dynamic, Eigen::Dynamic, Eigen::RowMajor>;
    std::vector<gtsam::Matrix> Gs;
    std::vector<gtsam::Vector> gs;
    size_t o = 0, go = 0;
    for (int i = 0; i < nkeys; ++i) // G11 G12 .. G1n G22 .. (photometric_factor.cpp:165-181)
      for (int j = i; j < nkeys; ++j)
      {
        Gs.emplace_back(Eigen::Map<const RowMajor>(G.data() + o, dims[i], dims[j]));
        o += (size_t)dims[i] * dims[j];
      }
    for (int i = 0; i < nkeys; ++i)
    {
      gs.emplace_back(Eigen::Map<const Eigen::VectorXd>(g.data() + go, dims[i]));
      go += dims[i];
    }
    return boost::make_shared<gtsam::HessianFactor>(factor_keys, Gs, gs, f); // f = error_ (photometric_factor.cpp:218)
  }

  SageWindow *win_;
  std::vector<Keys> keys_;
  int CS_, psd_mode_;
  bool device_psd_;
  std::vector<float> pose_, code_, scale_;
  std::mutex mutex_;

public:
  // >= 0: project every factor right after a batched linearisation on this many host threads (0 = the engine's default: a
  // quarter of the hardware threads, at most 64 -- include/sage_ba.h); -1: lazily, factor
  // by factor inside Linearize() (what ISAM2's partial relinearisation wants when it touches a few factors only)
  int eager_psd_threads_ = 0;
};

// In core/gtsam/photometric_factor.cpp the two bodies become (geometric_factor.cpp alike with type 1):
//
//   double PhotometricFactor<Scalar, CS>::error(const gtsam::Values &c) const
//   { return this->active(c) ? cache_->Error(c, 0, edge_) : 0.0; }
//
//   boost::shared_ptr<gtsam::GaussianFactor> PhotometricFactor<Scalar, CS>::linearize(const gtsam::Values &c) const
//   {
//     if (!this->active(c)) return boost::shared_ptr<gtsam::HessianFactor>();
//     return cache_->Linearize(c, 0, edge_, {pose0_key_, pose1_key_, code0_key_, scale0_key_});
//   }
//
// with two new members (std::shared_ptr<SageWindowCache> cache_; int edge_) set by Mapper when it adds the link.
//
// The matched-keypoint factor of a link direction and the factors of the loop-closure graphs carry the id their term got from
// sage_window_add_keypoint_term / sage_window_add_graph_term (int term_) instead of an edge; their bodies become
//
//   MatchGeometryFactor (core/gtsam/match_geometry_factor.cpp):
//     error:      return cache_->ErrorTerm(c, SAGE_TERM_KEYPOINT, term_);
//     linearize:  return cache_->LinearizeTerm(c, SAGE_TERM_KEYPOINT, SAGE_KP_MATCH_GEOMETRY, term_,
//                                              {pose0_key_, pose1_key_, code0_key_, code1_key_, scale0_key_, scale1_key_});
//   ReprojectionFactor (reprojection_factor.cpp):
//     error:      return cache_->ErrorTerm(c, SAGE_TERM_KEYPOINT, term_);
//     linearize:  return cache_->LinearizeTerm(c, SAGE_TERM_KEYPOINT, SAGE_KP_REPROJECTION, term_,
//                                              {pose0_key_, pose1_key_, code0_key_, scale0_key_});
//   LoopMGFactor (loop_mg_factor.cpp):
//     error:      return cache_->ErrorTerm(c, SAGE_TERM_KEYPOINT, term_);
//     linearize:  return cache_->LinearizeTerm(c, SAGE_TERM_KEYPOINT, SAGE_KP_LOOP_MG, term_,
//                                              {pose0_key_, pose1_key_, scale0_key_, scale1_key_});
//   RelPoseScaleFactor (rel_pose_scale_factor.cpp):
//     error:      return cache_->ErrorTerm(c, SAGE_TERM_GRAPH, term_);
//     linearize:  return cache_->LinearizeTerm(c, SAGE_TERM_GRAPH, SAGE_GRAPH_REL_POSE_SCALE, term_,
//                                              {pose0_key_, pose1_key_, scale0_key_, scale1_key_});
//   RelPoseFactor (rel_pose_factor.cpp):
//     error:      return cache_->ErrorTerm(c, SAGE_TERM_GRAPH, term_);
//     linearize:  return cache_->LinearizeTerm(c, SAGE_TERM_GRAPH, SAGE_GRAPH_REL_POSE, term_, {pose0_key_, pose1_key_});
//   ScaleFactor with a target (scale_factor.cpp):
//     error:      return cache_->ErrorTerm(c, SAGE_TERM_GRAPH, term_);
//     linearize:  return cache_->LinearizeTerm(c, SAGE_TERM_GRAPH, SAGE_GRAPH_SCALE_PRIOR, term_, {scale_key_});
//
// PoseFactor, CodeFactor and a ScaleFactor without a target are the window's priors: closed-form on the host, they stay as
// the reference wrote them.

} // namespace df
