// d2pc_sectors_steer.hip -- the kernel of the steer session of include/d2pc_sectors.h (gfx950).
//
// k_sectors_steer    ONE block of 1,024 lanes: the work is n_cells <= 5,760 cells of 16 bits, six a lane at the most, so
//                    launches and barriers are what it costs.  Two planes of 16-bit cells and the two reach tables live
//                    in LDS (27,312 bytes at the most).  (1) d into the first plane with the free_cm mapping, the tables
//                    beside it.  (2) Azimuth pass: a lane's cell takes the minimum of its row's neighbours that pass the
//                    row's reach_s entry, into the second plane; the lanes of a wave that share a layer read one LDS
//                    word per threshold (a broadcast).  (3) Layer pass over the second plane against reach_l: with (2)
//                    the direct 2-D window of the specification.  (4) Each lane forms the cost and the key
//                    (cost << 32) | cell of the cells it holds, in registers.  (5) The K smallest keys: K rounds of a
//                    block-wide minimum, ONE barrier a round; the rounds end with the first empty one.  A lane offers its
//                    smallest key not yet chosen (the keys are distinct); the wave takes the minimum of the costs and,
//                    among the lanes that hold it, of the cells -- two 32-bit minima over DPP row shifts and broadcasts,
//                    no LDS -- and one lane issues one 64-bit LDS min into the round's own word (K words, preset to all
//                    ones: nothing to reset, no word is used twice).  Behind the barrier every lane reads that word; the
//                    one lane whose key it is looks for its next.  The rounds are smallest_keys of
//                    d2pc_sectors_device.hpp, which the ground's and the terrain's sites call too.
//                    Vector stores only: no global atomic, nothing to clear.  Every value is an integer.
#include <hip/hip_runtime.h>

#include "d2pc_sectors_device.hpp"
#include "d2pc_sectors_steer_plan.hpp"

namespace d2pc {
namespace sectors {
namespace {

struct SteerArgs {   // SteerLaunch without its host-only members
  const uint16_t *distance_cm;
  const uint8_t *allowed;
  const uint32_t *step;
  const uint16_t *reach;
  uint16_t *clearance_cm;
  uint32_t *cost;
  unsigned long long *candidates;
  uint32_t *summary;
  int n_candidates;
  int n, layers, n_cells, wa, we;
  uint32_t free_cm, min_clearance_cm, horizon_cm, w_goal, w_prev, w_near;
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = uint32_t(__shfl_xor(int(v), m, 64));
    v = o < v ? o : v;
  }
  return v;
}

// D of the specification, times w; 0 when the sector switches the term off
__device__ __forceinline__ uint32_t turn_cost(uint32_t w, int s, int l, uint32_t to_sector, uint32_t to_layer, int n, int layers) {
  if (to_sector >= uint32_t(n)) return 0u;
  const int tl = to_layer >= uint32_t(layers) ? layers - 1 : int(to_layer);
  const int ds = s > int(to_sector) ? s - int(to_sector) : int(to_sector) - s;
  const int dl = l > tl ? l - tl : tl - l;
  return w * uint32_t((ds < n - ds ? ds : n - ds) + dl);
}

__global__ __launch_bounds__(kSteerThreads) void k_sectors_steer(const SteerArgs a) {
  extern __shared__ __align__(16) unsigned char lds[];
  __shared__ unsigned long long winner[D2PC_SECTORS_STEER_MAX_CANDIDATES];   // round r's own word
  if (threadIdx.x < D2PC_SECTORS_STEER_MAX_CANDIDATES) winner[threadIdx.x] = kNoKey;   // (two barriers lie before the first min into it)
  __shared__ uint32_t free_slot[kSteerWaves], near_slot[kSteerWaves];
  uint16_t *plane_d = reinterpret_cast<uint16_t *>(lds);       // d, after the free_cm mapping
  uint16_t *plane_a = plane_d + a.n_cells;                     // the azimuth pass's minima
  uint16_t *reach_s = plane_a + a.n_cells;                     // layers x (wa + 1)
  uint16_t *reach_l = reach_s + a.layers * (a.wa + 1);         // we + 1
  const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int row_words = a.wa + 1, n = a.n;

  // ---- (1) d and the tables into LDS
  uint32_t nearest = kSteerNothing;
  for (int c = tid; c < a.n_cells; c += kSteerThreads) {
    uint32_t v = a.distance_cm[c];
    v = v >= a.free_cm ? kSteerNothing : v;
    nearest = v < nearest ? v : nearest;
    plane_d[c] = uint16_t(v);
  }
  for (int j = tid; j < a.layers * row_words + a.we + 1; j += kSteerThreads) reach_s[j] = a.reach[j];   // (reach_l lies behind reach_s in both)
  const uint32_t goal_s = a.step[0], goal_l = a.step[1], prev_s = a.step[2], prev_l = a.step[3];
  __syncthreads();

  // ---- (2) the azimuth pass: row by row, against the row's own reach_s
  int sector[kSteerPerLane] = {}, layer[kSteerPerLane] = {};
#pragma unroll
  for (int k = 0; k < kSteerPerLane; ++k) {
    const int c = tid + k * kSteerThreads;
    if (c >= a.n_cells) continue;
    const int l = c / n, s = c - l * n, base = l * n;
    sector[k] = s, layer[k] = l;
    uint32_t m = plane_d[c];
    const uint16_t *row = reach_s + l * row_words;
    for (int j = 1; j <= a.wa; ++j) {
      const uint32_t thr = row[j];
      int right = s + j, left = s - j;
      right -= right >= n ? n : 0, left += left < 0 ? n : 0;    // (j <= n / 2: one turn at the most)
      const uint32_t vr = plane_d[base + right], vl = plane_d[base + left];
      m = vr <= thr && vr < m ? vr : m;
      m = vl <= thr && vl < m ? vl : m;
    }
    plane_a[c] = uint16_t(m);
  }
  __syncthreads();

  // ---- (3) the layer pass, (4) the cost and the key
  unsigned long long key[kSteerPerLane];
  uint32_t n_free = 0;
#pragma unroll
  for (int k = 0; k < kSteerPerLane; ++k) {
    key[k] = kNoKey;
    const int c = tid + k * kSteerThreads;
    if (c >= a.n_cells) continue;
    const int s = sector[k], l = layer[k];
    uint32_t m = plane_a[c];
    for (int j = 1; j <= a.we; ++j) {
      const uint32_t thr = reach_l[j];
      if (l + j < a.layers) {
        const uint32_t v = plane_a[c + j * n];
        m = v <= thr && v < m ? v : m;
      }
      if (l - j >= 0) {
        const uint32_t v = plane_a[c - j * n];
        m = v <= thr && v < m ? v : m;
      }
    }
    if (a.clearance_cm) a.clearance_cm[c] = uint16_t(m);
    const bool is_free = m >= a.min_clearance_cm && (!a.allowed || a.allowed[c] != 0);
    uint32_t cost = 0xFFFFFFFFu;
    if (is_free) {
      cost = turn_cost(a.w_goal, s, l, goal_s, goal_l, n, a.layers) + turn_cost(a.w_prev, s, l, prev_s, prev_l, n, a.layers) +
             a.w_near * (a.horizon_cm - (m < a.horizon_cm ? m : a.horizon_cm));
      key[k] = (static_cast<unsigned long long>(cost) << 32) | uint32_t(c);
      ++n_free;
    }
    if (a.cost) a.cost[c] = cost;
  }

  // ---- the summary: the free cells and the nearest d of the whole grid
  if (a.summary) {   // (uniform: a kernel argument)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) n_free += uint32_t(__shfl_xor(int(n_free), m, 64));
    nearest = wave_min(nearest);
    if (lane == 0) free_slot[wave] = n_free, near_slot[wave] = nearest;
    __syncthreads();
    if (tid == 0) {
      uint32_t total = 0, least = kSteerNothing;
      for (int w = 0; w < kSteerWaves; ++w) total += free_slot[w], least = near_slot[w] < least ? near_slot[w] : least;
      a.summary[0] = total, a.summary[1] = least, a.summary[2] = 0u, a.summary[3] = 0u;
    }
  }

  // ---- (5) the K smallest keys, ascending
  smallest_keys(key, a.n_candidates, winner, a.candidates);   // (d2pc_sectors_device.hpp)
}

}  // namespace

int launch_steer(const SteerLaunch &in) {
  SteerArgs a;
  a.distance_cm = in.distance_cm, a.allowed = in.allowed, a.step = static_cast<const uint32_t *>(in.step), a.reach = in.reach;
  a.clearance_cm = in.clearance_cm, a.cost = in.cost, a.candidates = static_cast<unsigned long long *>(in.candidates);
  a.summary = in.summary, a.n_candidates = in.candidates ? in.n_candidates : 0;
  const SteerPlan &p = in.plan;
  a.n = p.grid.n_sectors, a.layers = p.grid.n_layers, a.n_cells = p.grid.n_cells, a.wa = p.wa, a.we = p.we;
  a.free_cm = p.free_cm, a.min_clearance_cm = p.min_clearance_cm, a.horizon_cm = p.horizon_cm;
  a.w_goal = p.w_goal, a.w_prev = p.w_prev, a.w_near = p.w_near;
  // (the largest: two planes of 5,760 cells and 64 x 33 + 17 table words, 27,312 bytes: below the 64 KB a launch may ask for unannounced)
  void *args[] = {&a};
  (void)hipLaunchKernel(reinterpret_cast<const void *>(&k_sectors_steer), dim3(1), dim3(kSteerThreads), args, p.lds_bytes,
                        static_cast<hipStream_t>(in.stream));
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
