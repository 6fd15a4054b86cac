// d2pc_sectors_ground_sites.hpp -- what the ground's kernels (d2pc_sectors_ground.hip) and the terrain's
// (d2pc_sectors_terrain.hip) share on the device, each written once: the per-cell formula (floor mean, wrapped S) of a
// cell's count, sum and sum2, and the site stage of ONE block of kGroundSiteThreads lanes -- the direct (2W + 1)^2 walk,
// cost and key in registers, the summary from wave reductions, the K smallest keys by the steer's rounds.
// Device code: a .hip file includes it.  Every value is an integer: the result is the same bytes whatever the order.
#pragma once
#include <hip/hip_runtime.h>

#include "d2pc_sectors_device.hpp"
#include "d2pc_sectors_ground_plan.hpp"

namespace d2pc {
namespace sectors {

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
  GroundSiteGrid grid;
  int n_candidates;   // 0 without candidates
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
  const int n_cells = a.grid.n_cells, n_a = a.grid.n_a, n_b = a.grid.n_b, W = a.grid.window;
  if (tid < D2PC_SECTORS_GROUND_MAX_CANDIDATES) lds.winner[tid] = kNoKey;
  const bool measured = a.goal_i < uint32_t(n_a) && a.goal_j < uint32_t(n_b);
  uint32_t n_sites = 0;
  __syncthreads();

  unsigned long long key[kGroundPerLane];
#pragma unroll
  for (int k = 0; k < kGroundPerLane; ++k) {
    key[k] = kNoKey;
    const int c = tid + k * kGroundSiteThreads;
    if (c >= n_cells) continue;
    const int j = c / n_a, i = c - j * n_a;
    bool site = i - W >= 0 && i + W < n_a && j - W >= 0 && j + W < n_b && lds.flat[c] != 0 && (!a.allowed || a.allowed[c] != 0);
    if (site) {
      const int m = lds.mean_q[c], step = int(a.grid.max_step_q);
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
      const uint32_t cost = a.grid.w_dist * dist + a.grid.w_rough * (spread[k] < a.grid.rough_cap ? spread[k] : a.grid.rough_cap);
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

  // ---- the K smallest keys, ascending (the steer's rounds: d2pc_sectors_device.hpp)
  smallest_keys(key, a.n_candidates, lds.winner, a.candidates);
}

}  // namespace sectors
}  // namespace d2pc
