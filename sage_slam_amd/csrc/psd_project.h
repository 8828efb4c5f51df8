// psd_project.h -- what the batched Higham projection (psd_project.hip: sage_factor_psd_batch, the device half of
// sage_window_prepare_factors_device) shares between host and device: the round-robin schedule of the parallel cyclic
// Jacobi sweeps, the layout of a workgroup's LDS and the plan of a batch.  psd_project_host.cpp holds the host-only
// definitions (plan, argument checks, the public schedule function); nothing here needs a device.
#pragma once

#include <cstdint>

#include "sage_ba.h"

#if defined(__HIPCC__)
#define PSD_HD __host__ __device__
#else
#define PSD_HD
#endif

constexpr int kPsdLanesPerPair = 16; // lanes that share one rotation of a round
constexpr int kPsdDimStep = 16;      // the kernel is instantiated per capacity: D rounded up to a multiple of this
constexpr int kPsdSweepCap = 30;     // sweeps after which a matrix that has not converged reports status 1
constexpr int kPsdBumpCap = 60;      // rounds of the bump loop (sage_nearest_psd)
constexpr int kPsdWaveSlots = 64;    // doubles of the reductions' per-wave slots (two sums x at most 16 waves, rounded up)

// rounds of one sweep: every index meets every other one exactly once (D = 1: one round without a pair)
PSD_HD inline int psd_rounds(int D) { return (D & 1) ? D : D - 1; }

// pair `slot` (0 <= slot < D / 2) of round `round` (0 <= round < psd_rounds(D)): the circle method over n = D rounded up to
// even, index n - 1 fixed, the others rotating.  With D odd the fixed index is the one that does not exist: its partner
// sits the round out, the remaining D / 2 pairs are numbered from 0.  p < q.
PSD_HD inline void psd_round_pair(int D, int round, int slot, int *p, int *q)
{
  const int n = D + (D & 1), m = n - 1;
  const int i = (D & 1) ? slot + 1 : slot;
  int a, b;
  if (i == 0)
  {
    a = round % m;
    b = n - 1;
  }
  else
  {
    a = (round + i) % m;
    b = (round + m - i) % m;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

PSD_HD constexpr int psd_capacity(int D) { return (D + kPsdDimStep - 1) / kPsdDimStep * kPsdDimStep; }
PSD_HD constexpr int psd_stride(int D) { return D | 1; } // doubles per row: odd, so a column walk visits every bank pair
// lanes of the workgroup of capacity Dc: one group of kPsdLanesPerPair per pair, whole waves
PSD_HD constexpr int psd_threads(int Dc) { return ((Dc / 2) * kPsdLanesPerPair + 63) / 64 * 64; }
// doubles of a workgroup's LDS at capacity Dc: the work matrix and the eigenvectors (then A3 and the LDL^T copy), four
// vectors of Dc, the reductions' slots
PSD_HD constexpr int psd_lds_doubles(int Dc) { return 2 * Dc * (Dc | 1) + 4 * Dc + kPsdWaveSlots; }

struct PsdPlan
{
  int D = 0, n = 0, capacity = 0, threads = 0;
  int64_t lds_bytes = 0, device_bytes = 0, pinned_bytes = 0;
  int launches = 0;
};
// 1 <= D <= SAGE_PSD_MAX_DIM, n >= 0 (the caller has checked)
void psd_plan(int D, int n, PsdPlan *plan);
// SAGE_OK or SAGE_E_INVALID for the arguments of sage_factor_psd_batch; touches no device
int psd_check_args(const void *ws, int D, int n, const void *AtA_dev, const void *C_dev);
