// d2pc_sectors_ground_sites.hpp -- what the ground's kernels (d2pc_sectors_ground.hip) and the terrain's
// (d2pc_sectors_terrain.hip) share on the device, each written once: the per-cell formula (floor mean, wrapped S) of a
// cell's count, sum and sum2, and the site stage of ONE block of kGroundSiteThreads lanes -- the direct (2W + 1)^2 walk,
// cost and key in registers, the summary from wave reductions, the K smallest keys by the steer's rounds.
// Device code: a .hip file includes it.  Every value is an integer: the result is the same bytes whatever the order.
#pragma once
#include <hip/hip_runtime.h>

#include "d2pc_sectors_ground_plan.hpp"

namespace d2pc {
namespace sectors {

constexpr unsigned long long kGroundNoKey = ~0ull;

// the wave's minimum of a 32-bit word in every lane (d2pc_sectors_steer.hip's, copied: the steer shares no code with the
// ground); all 64 lanes are active at every call
__device__ __forceinline__ uint32_t ground_wave_umin(uint32_t v) {
#define D2PC_GROUND_DPP_MIN(ctrl, rows)                                                             \
  {                                                                                                 \
    const uint32_t o = uint32_t(__builtin_amdgcn_update_dpp(-1, int(v), ctrl, rows, 0xf, false));   \
    v = o < v ? o : v;                                                                              \
  }
  D2PC_GROUND_DPP_MIN(0x111, 0xf)
  D2PC_GROUND_DPP_MIN(0x112, 0xf)
  D2PC_GROUND_DPP_MIN(0x114, 0xf)
  D2PC_GROUND_DPP_MIN(0x118, 0xf)
  D2PC_GROUND_DPP_MIN(0x142, 0xa)
  D2PC_GROUND_DPP_MIN(0x143, 0xc)
#undef D2PC_GROUND_DPP_MIN
  return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}

// mean_q (as a uint32) and spread_q2 of a cell from its count, sum and sum2: floor division towards -inf, S in wrapping
// 64-bit arithmetic (exact for what ground calls accumulate); the empty cell's words for a count of 0
__device__ __forceinline__ void ground_cell_formula(uint32_t cnt, unsigned long long sum, unsigned long long sum2, uint32_t *mean_q,
                                                    uint32_t *spread_q2) {
  uint32_t mean = D2PC_SECTORS_GROUND_EMPTY_MEAN, spread = D2PC_SECTORS_GROUND_EMPTY_SPREAD;
  if (cnt != 0u) {
    const long long total = static_cast<long long>(sum), c = static_cast<long long>(cnt);
    long long m = total / c;
    m -= (total % c != 0 && total < 0) ? 1 : 0;   // floor division towards -inf
    const unsigned long long um = static_cast<unsigned long long>(m);
    const unsigned long long S = sum2 - 2ull * um * sum + static_cast<unsigned long long>(cnt) * um * um;   // wrapping: exact
    mean = uint32_t(int(m)), spread = uint32_t(S / static_cast<unsigned long long>(cnt));
  }
  *mean_q = mean, *spread_q2 = spread;
}

struct GroundSiteStage {   // what the site stage reads of a call beside the block's LDS
  int n_a, n_b, n_cells, window, n_candidates;   // n_candidates: 0 without candidates
  uint32_t max_step_q, w_dist, w_rough, rough_cap;
  uint32_t goal_i, goal_j;
  const uint8_t *allowed;
  uint8_t *site;
  unsigned long long *candidates;
  uint32_t *summary;
};

// The LDS of the block that runs the stage: the caller declares one and fills mean_q / flat of its cells (lane `tid`
// holds the cells tid + k * kGroundSiteThreads) before the call; the stage's first barrier publishes them.
struct GroundSiteLds {
  int mean_q[kGroundMaxCells];
  uint8_t flat[kGroundMaxCells];
  unsigned long long winner[D2PC_SECTORS_GROUND_MAX_CANDIDATES];   // round r's own word
  uint32_t slot[3][kGroundSiteWaves];
};

// All kGroundSiteThreads lanes of the block call it, under uniform control flow.  spread[k] is the spread_q2 of the lane's
// k-th cell; points and n_flat are the lane's own partial sums for the summary.
__device__ __forceinline__ void ground_site_stage(const GroundSiteStage &a, GroundSiteLds &lds, const uint32_t (&spread)[kGroundPerLane],
                                                  uint32_t points, uint32_t n_flat) {
  const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int n_cells = a.n_cells, n_a = a.n_a, n_b = a.n_b, W = a.window;
  if (tid < D2PC_SECTORS_GROUND_MAX_CANDIDATES) lds.winner[tid] = kGroundNoKey;
  const bool measured = a.goal_i < uint32_t(n_a) && a.goal_j < uint32_t(n_b);
  uint32_t n_sites = 0;
  __syncthreads();

  unsigned long long key[kGroundPerLane];
#pragma unroll
  for (int k = 0; k < kGroundPerLane; ++k) {
    key[k] = kGroundNoKey;
    const int c = tid + k * kGroundSiteThreads;
    if (c >= n_cells) continue;
    const int j = c / n_a, i = c - j * n_a;
    bool site = i - W >= 0 && i + W < n_a && j - W >= 0 && j + W < n_b && lds.flat[c] != 0 && (!a.allowed || a.allowed[c] != 0);
    if (site) {
      const int m = lds.mean_q[c], step = int(a.max_step_q);
      for (int dj = -W; dj <= W; ++dj)
        for (int di = -W; di <= W; ++di) {
          const int o = c + dj * n_a + di;
          if (lds.flat[o] == 0) site = false;   // (an empty cell's mean is 0x80000000: no difference is formed with it)
          if (site) {
            const int d = lds.mean_q[o] - m;   // of flat cells: |mean_q| <= 32767
            site = (d < 0 ? -d : d) <= step;
          }
        }
    }
    if (a.site) a.site[c] = site ? 1 : 0;
    if (site) {
      const int di = i - int(a.goal_i), dj = j - int(a.goal_j);
      const uint32_t dist = measured ? uint32_t(di * di + dj * dj) : 0u;
      const uint32_t cost = a.w_dist * dist + a.w_rough * (spread[k] < a.rough_cap ? spread[k] : a.rough_cap);
      key[k] = (static_cast<unsigned long long>(cost) << 32) | uint32_t(c);
      ++n_sites;
    }
  }

  // ---- the summary
  if (a.summary) {   // (uniform: a kernel argument)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      points += uint32_t(__shfl_xor(int(points), m, 64));
      n_flat += uint32_t(__shfl_xor(int(n_flat), m, 64));
      n_sites += uint32_t(__shfl_xor(int(n_sites), m, 64));
    }
    if (lane == 0) lds.slot[0][wave] = points, lds.slot[1][wave] = n_flat, lds.slot[2][wave] = n_sites;
    __syncthreads();
    if (tid == 0) {
      uint32_t t0 = 0, t1 = 0, t2 = 0;
      for (int w = 0; w < kGroundSiteWaves; ++w) t0 += lds.slot[0][w], t1 += lds.slot[1][w], t2 += lds.slot[2][w];
      a.summary[0] = t0, a.summary[1] = t1, a.summary[2] = t2, a.summary[3] = 0u;
    }
  }

  // ---- the K smallest keys, ascending (the steer's rounds)
  unsigned long long head = key[0];   // the lane's smallest key not yet chosen
#pragma unroll
  for (int k = 1; k < kGroundPerLane; ++k) head = key[k] < head ? key[k] : head;
  for (int r = 0; r < a.n_candidates; ++r) {
    const uint32_t head_cost = uint32_t(head >> 32), head_cell = uint32_t(head);   // (all ones for no key: no cost is)
    const uint32_t least = ground_wave_umin(head_cost);
    const uint32_t cell = ground_wave_umin(head_cost == least ? head_cell : 0xFFFFFFFFu);
    if (lane == 0 && least != 0xFFFFFFFFu) atomicMin(&lds.winner[r], (static_cast<unsigned long long>(least) << 32) | cell);
    __syncthreads();
    const unsigned long long best = lds.winner[r];   // (the same value in every lane)
    if (best == kGroundNoKey) {   // no site is left: all ones from here on
      if (tid < a.n_candidates - r) a.candidates[r + tid] = kGroundNoKey;
      break;
    }
    if (tid == 0) a.candidates[r] = best;
    if (head == best) {   // one lane of the block: its next key
      head = kGroundNoKey;
#pragma unroll
      for (int k = 0; k < kGroundPerLane; ++k) head = key[k] > best && key[k] < head ? key[k] : head;
    }
  }
}

}  // namespace sectors
}  // namespace d2pc
