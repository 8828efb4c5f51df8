// registration_plan.h -- (no HIP) the layout of a batch of scale votes (sage_robust_registration_batch): which problems vote,
// in which order they lie in the workspace, and how many launches the batch spends.  registration_host.cpp holds the one
// definition (registration_batch_plan); the public sage_robust_registration_batch_plan and the call in registration.hip
// both read it.
#pragma once

#include <cstdint>

#include "sage_ba.h"

struct RegBatchSegment // one voting problem (N >= 2)
{
  int row;       // the caller's index of the problem
  int N, pairs;  // pairs = N (N - 1) / 2
  int P;         // the power of two >= max(2 pairs, 4096) its sort runs over
  int n_tiles;   // scan tiles of 2048 that hold an endpoint: ceil(2 pairs / 2048) <= P / 2048
  int start;     // its first endpoint in keys / payload: a multiple of P (the segments lie by descending P)
  int pair0;     // its first pair in pairs
  int tile0;     // the scan tiles before it (the grid of the sums and the cost)
  int cblock0;   // the 256-pair blocks before it (the grid of the count)
  int64_t rows0;   // its tile rows in the tiles allocation, in bytes: [n_tiles] sums | [n_tiles + 1] offsets | [n_tiles] minima
  int64_t record0; // its pinned record, in bytes: 64 + 32 N
};

struct RegBatchPlan
{
  int n = 0; // segments
  RegBatchSegment seg[SAGE_REG_MAX_BATCH];
  int endpoints = 0, pairs = 0, tiles = 0, cblocks = 0; // the totals: start, pair0, tile0, cblock0 behind the last segment
  int sort_tile = 0;                                    // endpoints per workgroup of the sort's LDS stages
  int64_t keys_bytes = 0, payload_bytes = 0, pairs_bytes = 0, tiles_bytes = 0; // the four device allocations
  int64_t device_bytes = 0, pinned_bytes = 0;
  int launches = 0; // 0 when nothing votes; the single call's when one problem votes (it takes that path)
};

// (the tiles allocation: the segments' counters [n][4] int first, so that one memset clears them, then the segments' rows,
// 160 (P / 2048) + 64 bytes each)
constexpr int kRegSingleFixedLaunches = 6; // pairs, sums, offsets, cost, count, publish (which posts the ticket)
constexpr int kRegBatchFixedLaunches = 7;  // two or more voting problems: the ticket is a launch of its own

// the finish on the device (SAGE_REG_FINISH_DEVICE: reg_finish_kernel in registration.hip): one workgroup per voting problem,
// one launch behind the vote's, a pinned record of its own per problem behind the votes' records
constexpr int kRegFinishRecordHeader = 128; // R, t, the four counts
constexpr int kRegFinishLdsBytes = 49840;   // 48 KiB TIMs (later the translation's tile) + 688 of reduction rows
constexpr int64_t reg_finish_record_bytes(int N) { return kRegFinishRecordHeader + 8 * (int64_t)N; } // | list [N] int32 | mask [N] uint8 |

// endpoints per workgroup of the sort's LDS stages: 1024, or what SAGE_REG_SORT_TILE names (1024, 2048, 4096)
int registration_sort_tile();
// the launches of one bitonic sort over P endpoints with that tile (P >= 4096 >= tile, powers of two)
int registration_sort_launches(int P, int tile);
// N [B]: every entry in 0 .. SAGE_REG_MAX_POINTS, 0 <= B <= SAGE_REG_MAX_BATCH (the caller has checked)
void registration_batch_plan(const int32_t *N, int B, int sort_tile, RegBatchPlan *plan);
