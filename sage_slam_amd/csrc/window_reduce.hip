// window_reduce.hip -- sum over the ranks and read totals back: the window's collectives (the all-reduce hook, the emulated
// peers' share), the pinned mirror of the totals with its waits, the total error; and the one-line device copies / adds the
// host steps of an iteration enqueue between the big kernels.
#include "runtime_internal.h"

namespace sage
{

__global__ void copy_floats_kernel(const float *__restrict__ src, float *__restrict__ dst, int n)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dst[i] = src[i];
}

// dst += src (peer emulation: the contribution of the ranks that are not there)
__global__ void add_doubles_kernel(const double *__restrict__ src, double *__restrict__ dst, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dst[i] += src[i];
}

// the (reduced) totals -- tail of the packed buffer, error buffer (may be null) -> pinned host mirror.  One wave; the values,
// a workgroup barrier, then one system-scope release and the four tickets in the kernel's OWN slots (mirror[12..15];
// error_totals_kernel owns mirror[8..11]): the host spins on them instead of synchronising the stream
__global__ void mirror_totals_kernel(const double *__restrict__ tail, const double *__restrict__ err,
                                     double *__restrict__ mirror, double epoch)
{
  const int t = threadIdx.x;
  if (t < 4)
    mirror[t] = tail[t];
  else if (t < 8 && err)
    mirror[t] = err[t - 4];
  __syncthreads();
  if (t == 0)
  {
    __threadfence_system();
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<volatile double *>(mirror + 12 + i) = epoch;
  }
}

} // namespace sage

// (these two never were in the namespace: their symbols stay what profiles of earlier builds call them)
__global__ void copy_doubles_kernel(const double *__restrict__ src, double *__restrict__ dst, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    dst[i] = src[i];
}

__global__ void add_to_double_kernel(double *p, double v) { p[0] += v; }

// (a kernel, not hipMemcpyAsync: a device-to-device copy of 11 KB costs ~10 us of API time on the step's critical path)
int window_copy_floats(SageWindow *w, const float *src, float *dst, int n)
{
  hipLaunchKernelGGL(copy_floats_kernel, dim3((n + 255) / 256), dim3(256), 0, w->stream, src, dst, n);
  SAGE_HIP(hipGetLastError());
  return SAGE_OK;
}

void window_add_to_double(SageWindow *w, double *p, double v)
{
  hipLaunchKernelGGL(add_to_double_kernel, dim3(1), dim3(1), 0, w->stream, p, v);
}

// ---- collectives ----
// the hook's sum and nothing else (the Schur sequence's payloads: it has no peer emulation)
int window_collective(SageWindow *w, double *buf, size_t n)
{
  if (!w->dist.allreduce || w->dist.allreduce(buf, n, w->dist.allreduce_user))
    return SAGE_E_STATE;
  return SAGE_OK;
}

// peer emulation: the absent ranks' share of a sum, from table entry `iterate` (nothing without a table)
static int window_add_emulated_peers(SageWindow *w, double *buf, size_t n, int iterate)
{
  if (w->dist.emu_rest && w->dist.emu_n > 0)
  {
    const size_t np = sage_window_packed_count(w);
    const double *rest = w->dist.emu_rest + (size_t)(((iterate % w->dist.emu_n) + w->dist.emu_n) % w->dist.emu_n) * np;
    if (n == np)
      hipLaunchKernelGGL(add_doubles_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, w->stream, rest, buf, np);
    else if (n == 4) // error totals of a candidate: the tail of the absent ranks' system at that iterate
      hipLaunchKernelGGL(add_doubles_kernel, dim3(1), dim3(64), 0, w->stream, rest + np - 4, buf, (size_t)4);
    else
      return SAGE_E_UNSUPPORTED;
    SAGE_HIP(hipGetLastError());
  }
  return SAGE_OK;
}

// the window's all-reduce of n doubles in place
int window_allreduce(SageWindow *w, double *buf, size_t n, int iterate)
{
  const int rc = window_collective(w, buf, n);
  return rc ? rc : window_add_emulated_peers(w, buf, n, iterate);
}

// out of place: recv = sum over the ranks of send (n = the packed system).  Native RCCL reduces send -> recv directly; a
// plain in-place hook gets a device copy first
int window_allreduce_into(SageWindow *w, const double *send, double *recv, size_t n, int iterate)
{
  if (w->dist.allreduce2)
  {
    if (w->dist.allreduce2(send, recv, n, w->dist.allreduce_user))
      return SAGE_E_STATE;
  }
  else
  {
    hipLaunchKernelGGL(copy_doubles_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, w->stream, send, recv, n);
    SAGE_HIP(hipGetLastError());
    const int rc = window_collective(w, recv, n);
    if (rc)
      return rc;
  }
  return window_add_emulated_peers(w, recv, n, iterate);
}

// ---- the pinned mirror of the totals ----
// enqueue the mirror of the (reduced) totals and their tickets
int window_mirror_totals(SageWindow *w, bool with_err, const double *system)
{
  w->mirror.mirror_epoch += 1;
  hipLaunchKernelGGL(mirror_totals_kernel, dim3(1), dim3(64), 0, w->stream,
                     (system ? system : w->packed.as<double>()) + sage_window_packed_count(w) - 4,
                     with_err ? w->errbuf.as<double>() : nullptr,
                     w->mirror.h, (double)w->mirror.mirror_epoch);
  SAGE_HIP(hipGetLastError());
  return SAGE_OK;
}

bool window_wait_error_totals(SageWindow *w)
{
  return w->kernels_mirror_totals() && w->mirror.err_epoch != 0 &&
         w->mirror.wait(TotalsMirror::kErrorTickets, w->mirror.err_epoch);
}

bool window_wait_reduced_totals(SageWindow *w)
{
  return w->mirror.h != nullptr && w->mirror.wait(TotalsMirror::kMirrorTickets, w->mirror.mirror_epoch);
}

// wait for the totals of the last window_mirror_totals: spin on their tickets (with the kernels of a shard 8x shorter,
// the 20-30 us wake-up of a thread blocked in a stream synchronise would be 4 % of an iteration), take up the candidate
// -- a non-positive pivot of its factorisation shows up there (*not_psd) -- and synchronise only if the spin timed out
int window_wait_mirror(SageWindow *w, bool *not_psd)
{
  const bool idle = window_wait_reduced_totals(w);
  const int rc = window_sync_candidate(w, idle);
  if (rc && rc != SAGE_E_NOT_PSD)
    return rc;
  *not_psd = rc == SAGE_E_NOT_PSD;
  if (!idle)
    SAGE_HIP(hipStreamSynchronize(w->stream));
  return SAGE_OK;
}

// total error from the pinned mirror: the edge totals at mirror.h[at], mirror.h[at + 1] (kTail: a system's tail, kError: an error
// pass's totals) plus the prior terms at variable set `set`
double mirrored_error(const SageWindow *w, int at, int set)
{
  return w->mirror.h[at] + w->mirror.h[at + 1] + window_prior_error(w, set);
}

// ---- the total error ----
// stream_idle: the caller has seen the error pass's tickets (window_wait_error_totals) -- nothing to synchronise
int window_total_error(SageWindow *w, int from_linearize, double *err, bool stream_idle)
{
  if (!w || !w->finalized || !err)
    return SAGE_E_STATE;
  double t[4];
  int rcs = window_sync_candidate(w, stream_idle);
  if (rcs && rcs != SAGE_E_NOT_PSD)
    return rcs;
  // a failed factorisation only invalidates the CANDIDATE: the error at the linearisation point is still served
  const int rc_out = from_linearize ? SAGE_OK : rcs;
  if (w->kernels_mirror_totals())
  {
    // the kernels mirrored the totals into pinned host memory (the writers -- ap.tail_mirror, the error_totals mirror -- ask
    // the same predicate; a one-rank RCCL communicator or sage_window_set_allreduce leaves the mirror unwritten and takes
    // the copies below: ADVICE r5)
    if (!stream_idle)
      SAGE_HIP(hipStreamSynchronize(w->stream));
    *err = mirrored_error(w, from_linearize ? TotalsMirror::kTail : TotalsMirror::kError, from_linearize ? 0 : 1);
    return rc_out;
  }
  if (from_linearize)
  {
    const size_t off = sage_window_packed_count(w) - 4;
    SAGE_HIP(hipMemcpyAsync(t, w->packed.as<double>() + off, 4 * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  }
  else
    SAGE_HIP(hipMemcpyAsync(t, w->errbuf.p, 4 * sizeof(double), hipMemcpyDeviceToHost, w->stream));
  SAGE_HIP(hipStreamSynchronize(w->stream));
  *err = t[0] + t[1] + window_prior_error(w, from_linearize ? 0 : 1);
  return rc_out;
}

extern "C" int sage_window_total_error(SageWindow *w, int from_linearize, double *err)
{
  return window_total_error(w, from_linearize, err, false);
}
