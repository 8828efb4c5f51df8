// keyframe_prepare.h -- what a prepared keyframe is, without HIP: the part of a window's configuration its preparation depends
// on (the fingerprint), the layout of its one device allocation, the layout of a prepare call's scratch on the workspace, the
// device tables of the two batch kernels and the call's plan.  keyframe_prepare_host.cpp implements it; keyframe_prepare.hip
// holds the kernels and the calls; the handle itself (it owns device memory) is in runtime_internal.h.
#pragma once

#include <cstddef>
#include <cstdint>

#include "sage_ba.h"

namespace sage
{
namespace prep
{

// the process's sample-order switches, as sage_window_finalize reads them: SAGE_SAMPLE_TILE=WxH (default 8x8, 0x0 = raster walk;
// read once per process), SAGE_SAMPLE_PAD=0 turns the tile-padded order off (read at every call)
struct SampleSwitches
{
  int32_t tile_w, tile_h, pad;
};
SampleSwitches sample_switches();

// everything a preparation depends on besides the keyframe's own arrays: two preparations under bit-equal fingerprints
// of the same arrays hold the same bytes
struct Fingerprint
{
  SagePyramid pyr;
  int32_t FS;
  float photo_weights[SAGE_MAX_LEVELS];
  SampleSwitches sw;
};
Fingerprint fingerprint(const SageWindowConfig &cfg, const SampleSwitches &sw);
// bit for bit over what is used: levels, P, FS, the switches, and per level its offset, its camera and its weight
bool same_fingerprint(const Fingerprint &a, const Fingerprint &b);

// SAGE_OK, or SAGE_E_INVALID: what a prepare call refuses about a configuration (levels, P, FS, image size, level weights)
int check_config(const SageWindowConfig *cfg);

// ---- a handle's one device allocation: planes | locations | rays | pre-sampled features, each sub-array at a multiple of kAlign
constexpr size_t kAlign = 256;
struct Layout
{
  size_t cap;                                // sample slots: max(1, ceil(5 N / 4))
  size_t off_pk, off_loc, off_homo, off_f0s; // bytes from the allocation's start
  size_t bytes;
};
Layout layout(int FS, int P, int levels, int N);

// ---- device tables of the batch kernels
struct RepackItem // one plane: blockIdx.z of repack_planes_batch_kernel
{
  float *dst;       // [FS/4][P][4]
  const float *src; // [FS][P]
  int32_t axis;     // 0 features, 1 d/dx (x fx_l), 2 d/dy (x fy_l)
  int32_t reserved;
};
struct PresampleItem // one keyframe: blockIdx.z of presample_source_batch_kernel
{
  float *f0s;           // [L][FS/4][slots][4]
  const float *feat_pk; // its relaid feature plane
  const float *homo;    // [slots][3]
  int32_t slots;
  int32_t reserved;
};
constexpr size_t kSortItemBytes = 48; // room per SortItem (sage_internal.h; keyframe_prepare.hip asserts it fits)

// ---- a call's scratch on the workspace: the tables (one host-to-device copy: [0, table_bytes)), then what the kernels write
struct Scratch
{
  size_t off_sort, off_repack, off_presample, table_bytes;
  size_t off_pad, off_status, off_tiles, off_mark; // pad flags [B], status [2 B] and tile counts [B] (adjacent), mark planes [B][HW]
  size_t bytes;
};
Scratch scratch(int B, int HW);

// launches (the two fills of the sort included) and waits of a batch none of whose keyframes takes the padded order; a
// batch with one: one more of each.  They do not depend on B
constexpr int kLaunches = 6, kWaits = 2;

} // namespace prep
} // namespace sage
