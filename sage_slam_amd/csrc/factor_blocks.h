// factor_blocks.h -- the host definition of a gtsam HessianFactor cut from one of the engine's systems (factor_blocks.cpp, no
// HIP): a dense factor's per-edge system, or a window term's system in its term group's layout.  One shape, one projection,
// one cut; the public sage_factor_* / sage_term_factor_* calls (include/sage_ba.h) and the window's factor cache
// (window_factors.hip) are argument checks around them.
#pragma once
#include <stdint.h>

namespace sage
{
// A factor's keys in the reference's push order with their dims, and the columns [first, first + D_own) it owns of a system
// of D_group columns.  nk == 0: no such factor
struct FactorShape
{
  int nk = 0, dims[6] = {0, 0, 0, 0, 0, 0};
  int D_group = 0, first = 0, D_own = 0;
};
// dense type 0 (photometric, keys {p0,p1,c0,s0}) / 1 (geometric, keys {p0,p1,c0,c1,s0,s1}): the whole per-edge system
FactorShape dense_factor_shape(int type, int CS);
// a window term by family (SAGE_TERM_*) and kind (SAGE_KP_* / SAGE_GRAPH_*)
FactorShape term_factor_shape(int family, int kind, int CS);
// doubles of the packed upper blocks G11 G12 .. Gnn, or SAGE_E_INVALID
int factor_block_count(const FactorShape &s);
// the own D_own x D_own sub-matrix of a D_group-stride AtA, widened to double element by element in row order and projected:
// psd_mode 0 none, 1 Higham (sage_nearest_psd), 2 NearestPsd as the reference wrote it -> C_out [D_own][D_own]
int factor_psd(const FactorShape &s, const float *AtA, int psd_mode, double *C_out);
// the upper-triangular blocks in push order of a (projected) matrix C with row stride ldc whose entry (0, 0) is the first own
// column, and g = the own columns of the D_group-layout Atb; dims_out / nkeys_out may be null
int factor_cut(const FactorShape &s, const double *C, int ldc, const float *Atb, double *G_out, double *g_out,
               int32_t *dims_out, int32_t *nkeys_out);
// both: project, then cut
int factor_blocks(const FactorShape &s, const float *AtA, const float *Atb, int psd_mode, double *G_out, double *g_out,
                  int32_t *dims_out, int32_t *nkeys_out);
} // namespace sage
