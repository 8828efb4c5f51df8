// keyframe_prepare_host.cpp -- the host half of prepared keyframes (keyframe_prepare.h), no HIP: the configuration
// fingerprint and its comparison, the argument checks, the layouts of a handle's allocation and of a call's scratch, and
// the two ABI calls that touch no device: sage_keyframe_prepare_plan, sage_keyframe_config_matches.
#include "keyframe_prepare.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace sage
{
namespace prep
{

SampleSwitches sample_switches()
{
  // (the tile: once per process, like the walk order of sage_window_finalize)
  static const SampleSwitches tile = [] {
    int tw = 8, th = 8;
    if (const char *e = getenv("SAGE_SAMPLE_TILE"))
      if (sscanf(e, "%dx%d", &tw, &th) != 2 || tw < 1 || th < 1)
        tw = th = 0;
    return SampleSwitches{tw, th, 0};
  }();
  SampleSwitches sw = tile;
  const char *p = getenv("SAGE_SAMPLE_PAD");
  sw.pad = (tile.tile_w * tile.tile_h == 64 && !(p && atoi(p) == 0)) ? 1 : 0;
  return sw;
}

Fingerprint fingerprint(const SageWindowConfig &cfg, const SampleSwitches &sw)
{
  Fingerprint f;
  std::memset(&f, 0, sizeof(f));
  f.pyr = cfg.pyr;
  f.FS = cfg.FS;
  std::memcpy(f.photo_weights, cfg.photo_weights, sizeof(f.photo_weights));
  f.sw = sw;
  return f;
}

static bool same_bits(const void *a, const void *b, size_t n) { return std::memcmp(a, b, n) == 0; }

bool same_fingerprint(const Fingerprint &a, const Fingerprint &b)
{
  if (a.pyr.levels != b.pyr.levels || a.pyr.P != b.pyr.P || a.FS != b.FS || a.sw.tile_w != b.sw.tile_w ||
      a.sw.tile_h != b.sw.tile_h || a.sw.pad != b.sw.pad)
    return false;
  const int L = std::min<int>(std::max<int>(a.pyr.levels, 0), SAGE_MAX_LEVELS);
  for (int l = 0; l < L; ++l)
    if (a.pyr.level_offsets[l] != b.pyr.level_offsets[l] || !same_bits(&a.pyr.cam[l], &b.pyr.cam[l], sizeof(SageCamera)) ||
        !same_bits(&a.photo_weights[l], &b.photo_weights[l], sizeof(float)))
      return false;
  return true;
}

int check_config(const SageWindowConfig *cfg)
{
  if (!cfg)
    return SAGE_E_INVALID;
  const SagePyramid &p = cfg->pyr;
  if (p.levels < 1 || p.levels > SAGE_MAX_LEVELS || p.P < 1 || cfg->FS < 4 || cfg->FS % 4 != 0)
    return SAGE_E_INVALID;
  for (int l = 0; l < p.levels; ++l)
  {
    const SageCamera &c = p.cam[l];
    if (!(c.w >= 1.f) || !(c.h >= 1.f) || !(c.w <= 32768.f) || !(c.h <= 32768.f) || p.level_offsets[l] < 0 ||
        (long long)p.level_offsets[l] + (long long)(int)c.w * (int)c.h > p.P)
      return SAGE_E_INVALID; // (the kernels index a level at its offset with its size: every level lies inside [0, P))
    if (!(cfg->photo_weights[l] >= 0.f))
      return SAGE_E_INVALID; // a negative or NaN level weight
  }
  return SAGE_OK;
}

static size_t align_up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

Layout layout(int FS, int P, int levels, int N)
{
  Layout l;
  l.cap = std::max<size_t>(1, ((size_t)5 * (size_t)std::max(N, 0) + 3) / 4);
  l.off_pk = 0;
  l.off_loc = align_up((size_t)3 * FS * P * sizeof(float));
  l.off_homo = l.off_loc + align_up(l.cap * sizeof(int64_t));
  l.off_f0s = l.off_homo + align_up(l.cap * 3 * sizeof(float));
  l.bytes = l.off_f0s + align_up(l.cap * (size_t)levels * FS * sizeof(float));
  return l;
}

Scratch scratch(int B, int HW)
{
  Scratch s;
  s.off_sort = 0;
  s.off_repack = align_up((size_t)B * kSortItemBytes);
  s.off_presample = s.off_repack + align_up((size_t)3 * B * sizeof(RepackItem));
  s.table_bytes = s.off_presample + align_up((size_t)B * sizeof(PresampleItem));
  s.off_pad = s.table_bytes;
  s.off_status = s.off_pad + align_up((size_t)B * sizeof(int32_t));
  s.off_tiles = s.off_status + (size_t)2 * B * sizeof(int32_t);
  s.off_mark = align_up(s.off_tiles + (size_t)B * sizeof(int32_t));
  s.bytes = s.off_mark + align_up((size_t)B * HW * sizeof(int32_t));
  return s;
}

} // namespace prep
} // namespace sage

using namespace sage;

extern "C" int sage_keyframe_prepare_plan(const SageWindowConfig *cfg, const int32_t *N, int B, uint64_t *device_bytes,
                                          uint64_t *scratch_bytes, int *launches, int *waits)
{
  if (!cfg || !N || B < 1 || B > SAGE_PREPARE_MAX_BATCH)
    return SAGE_E_INVALID;
  if (int rc = prep::check_config(cfg))
    return rc;
  for (int b = 0; b < B; ++b)
    if (N[b] < 0)
      return SAGE_E_INVALID;
  if (device_bytes)
    for (int b = 0; b < B; ++b)
      device_bytes[b] = prep::layout(cfg->FS, cfg->pyr.P, cfg->pyr.levels, N[b]).bytes;
  if (scratch_bytes)
    *scratch_bytes = prep::scratch(B, (int)cfg->pyr.cam[0].w * (int)cfg->pyr.cam[0].h).bytes;
  if (launches)
    *launches = prep::kLaunches;
  if (waits)
    *waits = prep::kWaits;
  return SAGE_OK;
}

extern "C" int sage_keyframe_config_matches(const SageWindowConfig *a, const SageWindowConfig *b)
{
  if (!a || !b)
    return SAGE_E_INVALID;
  const prep::SampleSwitches sw = prep::sample_switches();
  return prep::same_fingerprint(prep::fingerprint(*a, sw), prep::fingerprint(*b, sw)) ? 1 : 0;
}
