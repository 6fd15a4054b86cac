// d2pc_sectors_device.hpp -- what the kernels of libd2pc_sectors.so share on the device, each written once: the marks of
// "no cell" and "no key", the wave reduction over DPP, the K smallest keys of a block (the steer's candidates, the
// ground's and the terrain's sites) and the walk over a call's shares of records (the grid's reduce and the ground's).
// Device code: a .hip file includes it.  Every value here is an integer: the result is the same bytes whatever the order.
#pragma once
#include <hip/hip_runtime.h>

#include "d2pc_sectors_plan.hpp"

namespace d2pc {
namespace sectors {

constexpr uint32_t kNone = 0xFFFFFFFFu;          // the cell of a record that takes no part
constexpr unsigned long long kNoKey = ~0ull;     // (cost << 32) | cell of no cell: no cost is all ones

// A reduction over the wave's 64 lanes, in every lane, without LDS: an inclusive scan along each row of 16 lanes (row_shr
// 1, 2, 4, 8; a lane with no source takes `identity`), lane 15 of rows 0 and 2 broadcast into rows 1 and 3, lane 31 into
// rows 2 and 3; lane 63 then holds all.  All 64 lanes must be active (the callers' control flow is uniform).
template <class Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v, const uint32_t identity, Op op) {
#define D2PC_SECTORS_DPP(ctrl, rows) v = op(v, uint32_t(__builtin_amdgcn_update_dpp(int(identity), int(v), ctrl, rows, 0xf, false)))
  D2PC_SECTORS_DPP(0x111, 0xf);   // row_shr:1
  D2PC_SECTORS_DPP(0x112, 0xf);   // row_shr:2
  D2PC_SECTORS_DPP(0x114, 0xf);   // row_shr:4
  D2PC_SECTORS_DPP(0x118, 0xf);   // row_shr:8
  D2PC_SECTORS_DPP(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
  D2PC_SECTORS_DPP(0x143, 0xc);   // row_bcast:31 into rows 2 and 3
#undef D2PC_SECTORS_DPP
  return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}

__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
  return wave_reduce(v, kNone, [](uint32_t a, uint32_t b) { return b < a ? b : a; });
}

// The n_candidates smallest of a block's keys, ascending, into candidates[]; kNoKey from the first round that finds none.
// All lanes of the block call it, under uniform control flow, each with its kKeys distinct keys (cost << 32) | cell, kNoKey
// for none.  winner[r] is round r's own word in LDS: the CALLER presets winner[0 .. n_candidates) to kNoKey, and at least
// one barrier lies between that preset and this call (the steer has two before the first min into it, the site stage
// one).  A round: a lane offers its smallest key not yet chosen; the wave takes the minimum of the costs and, among the
// lanes that hold it, of the cells -- two 32-bit minima over DPP, no LDS -- and one lane issues one 64-bit LDS min into
// the round's word (nothing to reset, no word is used twice).  ONE barrier a round; behind it every lane reads that
// word, and the one lane whose key it is looks for its next.
template <int kKeys>
__device__ __forceinline__ void smallest_keys(const unsigned long long (&key)[kKeys], int n_candidates, unsigned long long *winner,
                                              unsigned long long *candidates) {
  const int tid = int(threadIdx.x), lane = tid & 63;
  unsigned long long head = key[0];   // the lane's smallest key not yet chosen
#pragma unroll
  for (int k = 1; k < kKeys; ++k) head = key[k] < head ? key[k] : head;
  for (int r = 0; r < n_candidates; ++r) {
    const uint32_t head_cost = uint32_t(head >> 32), head_cell = uint32_t(head);   // (all ones for no key: no cost is)
    const uint32_t least = wave_umin(head_cost);
    const uint32_t cell = wave_umin(head_cost == least ? head_cell : kNone);
    if (lane == 0 && least != kNone) atomicMin(&winner[r], (static_cast<unsigned long long>(least) << 32) | cell);
    __syncthreads();
    const unsigned long long best = winner[r];   // (the same value in every lane)
    if (best == kNoKey) {   // no key is left: all ones from here on
      if (tid < n_candidates - r) candidates[r + tid] = kNoKey;
      break;
    }
    if (tid == 0) candidates[r] = best;
    if (head == best) {   // one lane of the block: its next key
      head = kNoKey;
#pragma unroll
      for (int k = 0; k < kKeys; ++k) head = key[k] > best && key[k] < head ? key[k] : head;
    }
  }
}

// The walk over a call's records (CloudWalk, d2pc_sectors_plan.hpp) in a reducing block of kThreads lanes: block b of
// `blocks` takes shares b, b + blocks, ... below w.shares; find_share places a share, share_record loads the lane's k-th
// record of it, k < kPerLane: four 16-byte loads in flight per lane.
// The form is the one of several that compiles to what the loop written out in each kernel compiled to (hipcc of ROCm 7,
// profiles/sectors_shared_resources.txt): k_ground_reduce keeps its 38 VGPRs and 88 SGPRs, k_sectors_reduce its instruction
// stream.  ONE function that fills rec[] and have[] and returns whether the share holds a record -- with the walk by
// reference or by value, with the arrays by reference or in a struct returned by value -- cost k_ground_reduce 10 VGPRs
// and 6 SGPRs (48 / 94) and the reduces 12 to 17 instructions, wherever its result steered a `continue`; the finder with
// a loader of the whole arrays cost it 3 VGPRs.  Where the CloudWalk comes from matters too: k_ground_reduce reads it
// from its arguments, which embed it; k_sectors_reduce makes it of eight fields of its own (d2pc_sectors.hip says why).
struct ShareAt {
  uint64_t first;    // the cloud's first record in `points`; the position of any record of the share fits 32 bits
  uint32_t i0, n;    // the share's first record in its cloud, and the cloud's count
};

// where `share` lies; false where it lies behind its cloud's count: the block has nothing to load
__device__ __forceinline__ bool find_share(const CloudWalk &w, uint64_t share, ShareAt *at) {
  uint64_t cloud = 0;
  uint32_t in_cloud = uint32_t(share);
  if (w.n_clouds > 1) {
    cloud = share / w.shares_per_cloud;
    in_cloud = uint32_t(share - cloud * w.shares_per_cloud);
  }
  uint32_t n = w.cloud_points;
  if (w.counts) {
    const uint32_t given = w.counts[cloud];
    n = given == 0xFFFFFFFFu ? 0u : min(given, w.cloud_points);
  }
  at->i0 = in_cloud * uint32_t(D2PC_SECTORS_SHARE_POINTS);   // (< 2^32: shares_per_cloud <= 2^22)
  at->n = n, at->first = cloud * w.stride;
  return at->i0 < n;
}

// record at.i0 + k * kThreads + tid of the share's cloud, all zeros and *have false where that lies at or behind the
// count; a 32-byte record is the load of its first half.  Its 32-bit position in `points` is share_position(at, tid, k)
__device__ __forceinline__ uint4 share_record(const CloudWalk &w, const ShareAt &at, uint32_t tid, int k, bool *have) {
  const uint32_t i = at.i0 + uint32_t(k * kThreads) + tid;   // (i0 + 1,023 <= 2^32 - 1: no wrap)
  *have = i < at.n;
  uint4 rec = make_uint4(0u, 0u, 0u, 0u);
  if (*have) rec = static_cast<const uint4 *>(w.points)[(at.first + i) * w.step16];
  asm volatile("" ::"v"(rec.w));   // keeps the load a whole 16-byte one (w is not used: it would shrink to 12)
  return rec;
}

__device__ __forceinline__ uint32_t share_position(const ShareAt &at, uint32_t tid, int k) {
  return uint32_t(at.first) + at.i0 + uint32_t(k * kThreads) + tid;
}

}  // namespace sectors
}  // namespace d2pc
