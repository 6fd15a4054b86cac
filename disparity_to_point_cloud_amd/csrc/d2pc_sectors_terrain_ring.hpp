// d2pc_sectors_terrain_ring.hpp -- what the terrain's kernel (d2pc_sectors_terrain.hip) and the relief's
// (d2pc_sectors_relief.hip) share on the device, each written once: steps 1, 3 and 4 of the TERRAIN block of
// include/d2pc_sectors.h -- the anchor of a frame, the slot choice from the 16-byte headers and the compacted list of the
// slots that take part -- computed identically by every lane (and every block) that reads the same headers.
// Device code: a .hip file includes it.  The two float products of the anchor are rounded once.
#pragma once
#include <hip/hip_runtime.h>

#include "d2pc_sectors_terrain_plan.hpp"

namespace d2pc {
namespace sectors {

struct TerrainAnchor {   // step 1
  uint32_t h0_bits;
  float h0;
  bool anchored;
  int ia0, jb0;   // both 0 when not anchored
};

// step 1 from the 20 words of a d2pc_sectors_ground_step: the same words in every lane
__device__ __forceinline__ TerrainAnchor terrain_anchor(const uint32_t *step, float inv_c) {
#pragma clang fp contract(off)
  TerrainAnchor t;
  t.h0_bits = step[14];
  const float a0 = __uint_as_float(step[12]), b0 = __uint_as_float(step[13]);
  t.h0 = __uint_as_float(t.h0_bits);
  const float ua = a0 * inv_c, ub = b0 * inv_c;
  t.anchored = fabsf(ua) <= kTerrainAnchorMax && fabsf(ub) <= kTerrainAnchorMax;   // (a NaN fails)
  t.ia0 = t.anchored ? int(rintf(ua)) : 0, t.jb0 = t.anchored ? int(rintf(ub)) : 0;   // half to even
  return t;
}

struct TerrainSlot {   // step 3
  uint32_t largest, q;   // the largest seq of headers 0 .. depth - 1; the new one
  int v;                 // the replaced slot
  bool restart;          // the largest seq is 0xFFFFFFFF: all slots are first taken as empty
};

// step 3 from the headers in LDS, identically in every lane
__device__ __forceinline__ TerrainSlot terrain_slot_choice(const uint4 *hdr, int depth) {
  TerrainSlot t;
  uint32_t largest = 0u, smallest = 0xFFFFFFFFu;
  int v = 0;
  for (int s = 0; s < depth; ++s) {
    const uint32_t seq = hdr[s].w;
    largest = seq > largest ? seq : largest;
    if (seq < smallest) smallest = seq, v = s;   // (the lowest index on a tie)
  }
  t.largest = largest;
  t.restart = largest == 0xFFFFFFFFu;
  t.v = t.restart ? 0 : v;
  t.q = t.restart ? 1u : largest + 1u;
  return t;
}

// step 4: the slots that take part (seq != 0, the same h0, a shift that leaves some of the grid in sight), compacted into
// part_slot / part_di / part_dj and counted in *part_n, all in LDS.  The 64 lanes of ONE whole wave call it with lane =
// 0 .. 63 (the ballot is whole); the caller's next barrier publishes the list.
__device__ __forceinline__ void terrain_participants(const uint4 *hdr, int depth, int n_a, int n_b, const TerrainAnchor &an, const TerrainSlot &sl,
                                                     int lane, int *part_slot, int *part_di, int *part_dj, int *part_n) {
  bool takes = false;
  long long di = 0, dj = 0;
  if (an.anchored && !sl.restart && lane < depth && lane != sl.v) {
    const uint4 h = hdr[lane];
    di = static_cast<long long>(an.ia0) - static_cast<long long>(int(h.x));
    dj = static_cast<long long>(an.jb0) - static_cast<long long>(int(h.y));
    takes = h.w != 0u && __uint_as_float(h.z) == an.h0 && di > -n_a && di < n_a && dj > -n_b && dj < n_b;
  }
  const unsigned long long m = __ballot(takes);
  if (takes) {
    const int pos = __popcll(m & ((1ull << lane) - 1ull));   // (< 15: at most depth - 1 lanes take)
    part_slot[pos] = lane, part_di[pos] = int(di), part_dj[pos] = int(dj);
  }
  if (lane == 0) *part_n = __popcll(m);
}

}  // namespace sectors
}  // namespace d2pc
