// d2pc_sectors_bin.hpp -- where a record falls: the device code k_sectors_reduce (d2pc_sectors.hip) and
// k_sectors_memory_update (d2pc_sectors_memory.hip) share, so that the same statements put a remembered point and a
// cloud's point into a cell.  The kernels keep their loads, which records take part, the pose and the tables of cells.
// Every float expression is rounded once: contraction is off in every function here, sqrtf is the correctly rounded one.
#pragma once
#include <hip/hip_runtime.h>

#include "d2pc_sectors_device.hpp"

namespace d2pc {
namespace sectors {

struct GridArgs {   // Plan without its host-only members
  int n_sectors, n_layers, n_cells, half;
  float rmin2, rmax2, u_min, u_max, inv_h;
  int axis[3];
  uint32_t flip[3];
  uint32_t min_count, no_obstacle_cm;
};

inline GridArgs grid_args(const Plan &p) {
  GridArgs g;
  g.n_sectors = p.n_sectors, g.n_layers = p.n_layers, g.n_cells = p.n_cells, g.half = p.half;
  g.rmin2 = p.rmin2, g.rmax2 = p.rmax2, g.u_min = p.u_min, g.u_max = p.u_max, g.inv_h = p.inv_h;
  for (int i = 0; i < 3; ++i) g.axis[i] = p.axis[i], g.flip[i] = p.flip[i];
  g.min_count = p.min_count, g.no_obstacle_cm = p.no_obstacle_cm;
  return g;
}

// `Record` is how a record reaches these functions, `const uint4 &` or `uint4`: the same statements either way, but
// hipcc (ROCm 7) allocates k_sectors_reduce 68 VGPRs with the reference and 80 with the value, and
// k_sectors_memory_update<HEIGHT> 67 with the value and 99 with the reference.  Each kernel names the one it had.
template <class Record>
__device__ __forceinline__ float pick(Record p, int axis, uint32_t flip) {
  return __uint_as_float((axis == 0 ? p.x : axis == 1 ? p.y : p.z) ^ flip);
}

// A record behind its step.  The kernels copy the fields into one array per field and keep the two loops over the
// boundaries in their own bodies: one aggregate, or the loops in a function, cost hipcc (ROCm 7) 20 VGPRs and more.
struct Binned {
  float f, l;          // behind the half turn
  float up, hz;        // elevation: u and the horizontal range h = sqrtf(r2)
  uint32_t cell;       // kNone, or the layer's first cell (0 for elevation layers: cell_of adds the layer)
  uint32_t sector;     // n_sectors / 2 in the half turn behind the first boundary, else 0: the count of boundaries adds the rest
  uint32_t key_bits;   // bits(r2), or bits(d2) for elevation layers
};

// One record's step.  `take`: the kernel's own reason to look at the record at all; t0: the first azimuth boundary,
// tab[0]; lo, hi: the elevation band's two boundaries, tab[half] and tab[half + n_layers] (unused for height layers)
template <bool kElevation, class Record>
__device__ __forceinline__ Binned bin_record(const GridArgs g, const float2 t0, const float2 lo, const float2 hi, Record p, bool take) {
#pragma clang fp contract(off)
  Binned b;
  b.up = b.hz = 0.0f;
  const bool finite = (p.x & 0x7F800000u) != 0x7F800000u && (p.y & 0x7F800000u) != 0x7F800000u && (p.z & 0x7F800000u) != 0x7F800000u;
  const float ff = pick<Record>(p, g.axis[0], g.flip[0]), ll = pick<Record>(p, g.axis[1], g.flip[1]);
  const float u = pick<Record>(p, g.axis[2], g.flip[2]);
  const float r2 = ff * ff + ll * ll;
  bool in;
  uint32_t layer = 0;
  float key = r2;
  if constexpr (kElevation) {
    // the band's two boundaries are gates; `!(t >= 0)` and `t >= 0` as written: a NaN t (0 * inf) takes no part
    const float h = __builtin_sqrtf(r2);   // (the correctly rounded one: the file's flags)
    key = r2 + u * u;
    const float t_lo = lo.x * u - lo.y * h, t_hi = hi.x * u - hi.y * h;
    in = take && finite && r2 > 0.0f && key >= g.rmin2 && key <= g.rmax2 && t_lo >= 0.0f && !(t_hi >= 0.0f);
    b.up = u, b.hz = h;
  } else {
    in = take && finite && r2 > 0.0f && r2 >= g.rmin2 && r2 <= g.rmax2 && u >= g.u_min && u < g.u_max;
    if (g.n_layers > 1) {
      const float slab = floorf((u - g.u_min) * g.inv_h);
      layer = slab >= float(g.n_layers - 1) ? uint32_t(g.n_layers - 1) : uint32_t(int(slab));   // (in: slab >= 0)
    }
  }
  const float cross0 = t0.x * ll - t0.y * ff, dot0 = t0.x * ff + t0.y * ll;
  // the half turn as a sign-bit mask, without a branch: hipcc of ROCm 7 structurised `if (A || (B && C)) negate` so
  // that the lanes of B && C kept f and l un-negated (tests/test_sectors_gpu.py: l = +-0 with f < 0)
  const uint32_t turn = (uint32_t(cross0 < 0.0f) | (uint32_t(cross0 == 0.0f) & uint32_t(dot0 < 0.0f))) << 31;
  b.f = __uint_as_float(__float_as_uint(ff) ^ turn), b.l = __uint_as_float(__float_as_uint(ll) ^ turn);
  b.sector = turn ? uint32_t(g.half) : 0u;
  b.cell = in ? layer * uint32_t(g.n_sectors) : kNone;
  b.key_bits = __float_as_uint(key);
  return b;
}

// One step of either count of boundaries: 1 where the record lies at or behind the boundary t, a compare folded into an
// add.  A kernel's loop reads t from LDS once for the lane's records (a broadcast: no bank conflict): the azimuth table's
// j = 1 .. half - 1 against (l, f) into `sector`, the elevation table's tab[half + i], i = 1 .. n_layers - 1, against
// (up, hz) into the layer.
__device__ __forceinline__ uint32_t behind(const float2 t, float x, float y) {
#pragma clang fp contract(off)
  return (t.x * x - t.y * y) >= 0.0f ? 1u : 0u;
}

// the record's cell behind both counts (< n_cells: counts of boundaries), or kNone; `layer` is the elevation count
__device__ __forceinline__ uint32_t cell_of(const GridArgs &g, uint32_t cell, uint32_t sector, uint32_t layer) {
  return cell == kNone ? kNone : cell + sector + layer * uint32_t(g.n_sectors);
}

// the range a cell's key holds
__device__ __forceinline__ float range_of_key(unsigned long long key) {
  return __builtin_sqrtf(__uint_as_float(uint32_t(key >> 32)));
}

// distance_cm of a cell: the clamp is taken in float, before the conversion
__device__ __forceinline__ uint16_t distance_cm_of(const GridArgs &g, float range, bool none) {
#pragma clang fp contract(off)
  const float cm = range * 100.0f;
  return uint16_t(none ? g.no_obstacle_cm : cm >= 65534.0f ? 65534u : uint32_t(cm));
}

}  // namespace sectors
}  // namespace d2pc
