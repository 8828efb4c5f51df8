// factor_blocks.cpp -- HessianFactor blocks (a6 / a7) of a dense factor's per-edge system and of a window term's system: the
// shapes, the projection of a factor's own matrix, the cut into the reference's G11 G12 .. Gnn / g1 .. gn order
// (photometric_factor.cpp:142-181).  Pure CPU.
//
//   sage_factor_block_count, sage_factor_psd, sage_factor_cut_blocks, sage_factor_hessian_blocks   a dense type's
//   sage_term_factor_block_count, sage_term_factor_blocks                                          a window term's
#include <cstring>
#include <initializer_list>
#include <vector>

#include "factor_blocks.h"
#include "sage_ba.h"

namespace sage
{
static void set_shape(FactorShape &s, std::initializer_list<int> dims, int D_group, int first)
{
  for (int v : dims)
  {
    s.dims[s.nk++] = v;
    s.D_own += v;
  }
  s.D_group = D_group;
  s.first = first;
}

FactorShape dense_factor_shape(int type, int CS)
{
  FactorShape s;
  if (CS < 1)
    return s;
  if (type == 0)
    set_shape(s, {6, 6, CS, 1}, 13 + CS, 0);
  else if (type == 1)
    set_shape(s, {6, 6, CS, CS, 1, 1}, 14 + 2 * CS, 0);
  return s;
}

// The keys in the reference's push order (MatchGeometryFactor, ReprojectionFactor, LoopMGFactor, RelPoseScaleFactor,
// RelPoseFactor, ScaleFactor), the columns of the term group's layout the kind owns -- the reference projects a
// RelPoseFactor's 12 x 12 and a ScaleFactor's 1 x 1, not the zero-padded 14 x 14 the window keeps them in.  The two keypoint
// kinds that fill a dense layout are the dense types
FactorShape term_factor_shape(int family, int kind, int CS)
{
  FactorShape s;
  if (CS < 1 || (family != SAGE_TERM_KEYPOINT && family != SAGE_TERM_GRAPH))
    return s;
  if (family == SAGE_TERM_KEYPOINT)
  {
    if (kind == SAGE_KP_REPROJECTION)
      return dense_factor_shape(0, CS);
    if (kind == SAGE_KP_MATCH_GEOMETRY)
      return dense_factor_shape(1, CS);
    if (kind == SAGE_KP_LOOP_MG)
      set_shape(s, {6, 6, 1, 1}, 14, 0);
  }
  else
  {
    if (kind == SAGE_GRAPH_REL_POSE_SCALE)
      set_shape(s, {6, 6, 1, 1}, 14, 0);
    else if (kind == SAGE_GRAPH_REL_POSE)
      set_shape(s, {6, 6}, 14, 0);
    else if (kind == SAGE_GRAPH_SCALE_PRIOR)
      set_shape(s, {1}, 14, 12);
  }
  return s;
}

int factor_block_count(const FactorShape &s)
{
  if (!s.nk)
    return SAGE_E_INVALID;
  int total = 0;
  for (int i = 0; i < s.nk; ++i)
    for (int j = i; j < s.nk; ++j)
      total += s.dims[i] * s.dims[j];
  return total;
}

int factor_psd(const FactorShape &s, const float *AtA, int psd_mode, double *C_out)
{
  if (!s.nk || !AtA || !C_out || psd_mode < 0 || psd_mode > 2)
    return SAGE_E_INVALID;
  const int D = s.D_own;
  std::vector<double> M((size_t)D * D);
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) // AtA_.cast<double>() (photometric_factor.cpp:305, :142)
      M[(size_t)i * D + j] = (double)AtA[(size_t)(s.first + i) * s.D_group + s.first + j];
  if (psd_mode == 1)
    return sage_nearest_psd(M.data(), D, C_out);
  if (psd_mode == 2)
    return sage_nearest_psd_reference(M.data(), D, C_out);
  std::memcpy(C_out, M.data(), M.size() * sizeof(double));
  return SAGE_OK;
}

int factor_cut(const FactorShape &s, const double *C, int ldc, const float *Atb, double *G_out, double *g_out,
               int32_t *dims_out, int32_t *nkeys_out)
{
  if (!s.nk || !C || !Atb || !G_out || !g_out || ldc < s.D_own)
    return SAGE_E_INVALID;
  int off[6], D = 0;
  for (int i = 0; i < s.nk; ++i)
  {
    off[i] = D;
    D += s.dims[i];
  }
  double *o = G_out;
  for (int i = 0; i < s.nk; ++i)
    for (int j = i; j < s.nk; ++j)
      for (int r = 0; r < s.dims[i]; ++r)
        for (int c = 0; c < s.dims[j]; ++c)
          *o++ = C[(size_t)(off[i] + r) * ldc + off[j] + c];
  for (int i = 0; i < D; ++i)
    g_out[i] = (double)Atb[s.first + i];
  if (dims_out)
    for (int i = 0; i < s.nk; ++i)
      dims_out[i] = s.dims[i];
  if (nkeys_out)
    *nkeys_out = s.nk;
  return SAGE_OK;
}

int factor_blocks(const FactorShape &s, const float *AtA, const float *Atb, int psd_mode, double *G_out, double *g_out,
                  int32_t *dims_out, int32_t *nkeys_out)
{
  if (!s.nk || !AtA || !Atb || !G_out || !g_out || psd_mode < 0 || psd_mode > 2)
    return SAGE_E_INVALID;
  std::vector<double> C((size_t)s.D_own * s.D_own);
  const int rc = factor_psd(s, AtA, psd_mode, C.data());
  return rc ? rc : factor_cut(s, C.data(), s.D_own, Atb, G_out, g_out, dims_out, nkeys_out);
}
} // namespace sage

using namespace sage;

extern "C" int sage_factor_block_count(int type, int CS) { return factor_block_count(dense_factor_shape(type, CS)); }

extern "C" int sage_factor_psd(int type, int CS, const float *AtA, int psd_mode, double *C_out)
{
  return factor_psd(dense_factor_shape(type, CS), AtA, psd_mode, C_out);
}

extern "C" int sage_factor_cut_blocks(int type, int CS, const double *C, const float *Atb, double *G_out, double *g_out,
                                      int32_t *dims_out, int32_t *nkeys_out)
{
  const FactorShape s = dense_factor_shape(type, CS);
  return factor_cut(s, C, s.D_own, Atb, G_out, g_out, dims_out, nkeys_out);
}

extern "C" int sage_factor_hessian_blocks(int type, int CS, const float *AtA, const float *Atb, int psd_mode,
                                          double *G_out, double *g_out, int32_t *dims_out, int32_t *nkeys_out)
{
  return factor_blocks(dense_factor_shape(type, CS), AtA, Atb, psd_mode, G_out, g_out, dims_out, nkeys_out);
}

extern "C" int sage_term_factor_block_count(int family, int kind, int CS)
{
  return factor_block_count(term_factor_shape(family, kind, CS));
}

extern "C" int sage_term_factor_blocks(int family, int kind, int CS, const float *AtA, const float *Atb, int psd_mode,
                                       double *G_out, double *g_out, int32_t *dims_out, int32_t *nkeys_out)
{
  return factor_blocks(term_factor_shape(family, kind, CS), AtA, Atb, psd_mode, G_out, g_out, dims_out, nkeys_out);
}
