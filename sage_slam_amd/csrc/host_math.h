// host_math.h -- internal host-side dense helpers (double precision), stateless.  The block solver of the window's
// normal equations has a unit of its own: block_solver.h.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace sage
{
// boolean environment switch ("Environment switches"): set and neither empty nor "0"
inline bool env_flag(const char *name)
{
  const char *e = getenv(name);
  return e && e[0] && !(e[0] == '0' && e[1] == 0);
}

void sym_eig(std::vector<double> &A, int n, std::vector<double> &w, std::vector<double> &V);
void rotation_to_angle_axis_as_reference(const float *R, float eps, float *out);

// A window term's factor by family (SAGE_TERM_*) and kind: its keys in the reference's push order with their dims, and the
// columns [first, first + D_own) it owns of its term group's D_group-column layout.  nk == 0: no such family / kind / CS
struct TermShape
{
  int nk = 0, dims[6] = {0, 0, 0, 0, 0, 0};
  int D_group = 0, first = 0, D_own = 0;
};
TermShape term_shape(int family, int kind, int CS);
// the two halves of sage_term_factor_blocks: the kind's own D_own x D_own sub-matrix of a group-layout AtA, widened and
// projected per psd_mode (C_out [D_own][D_own]); the upper blocks in push order of a matrix C with row stride ldc whose entry
// (0, 0) is the kind's first own column, and g = the kind's columns of the group-layout Atb
int term_factor_psd(int family, int kind, int CS, const float *AtA, int psd_mode, double *C_out);
int term_factor_cut(int family, int kind, int CS, const double *C, int ldc, const float *Atb, double *G_out, double *g_out,
                    int32_t *dims_out, int32_t *nkeys_out);
} // namespace sage
