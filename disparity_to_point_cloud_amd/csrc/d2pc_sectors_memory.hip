// d2pc_sectors_memory.hip -- the kernels of the memory session of include/d2pc_sectors.h (gfx950).
//
// k_sectors_memory_update   ONE block of 1,024 lanes: the work is n_cells <= 5,760 records of 16 bytes, not a cloud.
//                    The carry table (one 64-bit key a cell, <= 46,080 bytes) and the azimuth / elevation tables live in
//                    LDS.  Carry: a lane takes kMemoryPerLane remembered records of buffer `parity` per pass, ages them,
//                    moves them into the frame of `points` (the transpose of R on w - t) and bins them exactly as
//                    k_sectors_reduce bins a record: the same picks, gates, half turn (the branch-free sign mask) and
//                    counts of boundaries, one broadcast LDS read per boundary serving the lane's records; the key
//                    (bits(k) << 32) | record goes into the cell with one 64-bit LDS min.  Merge: a lane takes a cell; a
//                    fresh cell reads its nearest point and moves it to the world, a remembered one copies the record the
//                    key names, and the lane stores the new record to buffer 1 - parity and the outputs asked for.  The
//                    parity word is flipped on the device by the last store, so a replayed graph advances as plain calls.
//                    Vector stores only: no global atomic, nothing to clear.
// k_sectors_memory_reset    stores the empty record over both buffers.
// Every float expression of the specification is rounded once: contraction is off in this file, sqrtf is the correctly
// rounded one (SECTORS_FLAGS).
#include <hip/hip_runtime.h>

#include "d2pc_sectors_memory_plan.hpp"

namespace d2pc {
namespace sectors {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;   // a record that takes no part

struct MemoryArgs {   // MemoryLaunch without its host-only members
  const uint4 *points;
  const uint32_t *count, *nearest, *step;
  const uint8_t *covered;
  const float2 *table;
  uint4 *buffers;
  uint32_t *parity;
  float *range;
  uint16_t *distance_cm;
  uint32_t *age;
  uint4 *records;
  uint32_t bound, step16, max_age, min_count, no_obstacle_cm;
  int n_sectors, n_layers, n_cells, half;
  float rmin2, rmax2, u_min, u_max, inv_h;
  int axis[3];
  uint32_t flip[3];
};

__device__ __forceinline__ float pick(uint32_t x, uint32_t y, uint32_t z, int axis, uint32_t flip) {
  return __uint_as_float((axis == 0 ? x : axis == 1 ? y : z) ^ flip);
}

// a' = min(a + dt, 0xFFFFFFFE) without wrap
__device__ __forceinline__ uint32_t aged(uint32_t a, uint32_t dt) {
  const unsigned long long s = static_cast<unsigned long long>(a) + dt;
  return s > kOldestAge ? kOldestAge : uint32_t(s);
}

template <int kKind>
__global__ __launch_bounds__(kMemoryThreads) void k_sectors_memory_update(const MemoryArgs a) {
#pragma clang fp contract(off)
  constexpr bool kElevation = kKind == D2PC_SECTORS_LAYERS_ELEVATION;
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned long long *carry = reinterpret_cast<unsigned long long *>(lds);
  float2 *tab = reinterpret_cast<float2 *>(carry + a.n_cells);
  [[maybe_unused]] const float2 *etab = tab + a.half;   // n_layers + 1 x (ce, se), behind the azimuth table
  const uint32_t tid = threadIdx.x;
  for (int i = int(tid); i < a.n_cells; i += kMemoryThreads) carry[i] = ~0ull;
  for (int j = int(tid); j < a.half + (kElevation ? a.n_layers + 1 : 0); j += kMemoryThreads) tab[j] = a.table[j];
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = __uint_as_float(a.step[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = __uint_as_float(a.step[9 + i]);
  const uint32_t dt = a.step[12];
  const uint32_t par = *a.parity & 1u;   // (read by every lane before the barriers; lane 0 stores it behind the last one)
  const uint4 *src = a.buffers + size_t(par) * size_t(a.n_cells);
  uint4 *dst = a.buffers + size_t(par ^ 1u) * size_t(a.n_cells);
  __syncthreads();

  // ---- carry: the remembered records of `src` into the cells they fall into under the new pose
  for (int base = 0; base < a.n_cells; base += kMemoryThreads * kMemoryPerLane) {
    if (base + int(tid & ~63u) >= a.n_cells) continue;   // wave-uniform: none of this wave's records exists
    float f[kMemoryPerLane], l[kMemoryPerLane];
    uint32_t cell[kMemoryPerLane], key_bits[kMemoryPerLane], sector[kMemoryPerLane];
    [[maybe_unused]] float up[kMemoryPerLane], hz[kMemoryPerLane];
    const float2 t0 = tab[0];
    [[maybe_unused]] float2 lo, hi;
    if constexpr (kElevation) lo = etab[0], hi = etab[a.n_layers];
#pragma unroll
    for (int k = 0; k < kMemoryPerLane; ++k) {
      const int i = base + k * kMemoryThreads + int(tid);
      uint4 w = make_uint4(0u, 0u, 0u, kEmptyAge);
      if (i < a.n_cells) w = src[i];
      const bool kept = w.w != kEmptyAge && aged(w.w, dt) <= a.max_age;
      const float dx = __uint_as_float(w.x) - t[0], dy = __uint_as_float(w.y) - t[1], dz = __uint_as_float(w.z) - t[2];
      const uint32_t px = __float_as_uint(R[0] * dx + R[3] * dy + R[6] * dz);
      const uint32_t py = __float_as_uint(R[1] * dx + R[4] * dy + R[7] * dz);
      const uint32_t pz = __float_as_uint(R[2] * dx + R[5] * dy + R[8] * dz);
      const bool finite = (px & 0x7F800000u) != 0x7F800000u && (py & 0x7F800000u) != 0x7F800000u && (pz & 0x7F800000u) != 0x7F800000u;
      const float ff = pick(px, py, pz, a.axis[0], a.flip[0]), ll = pick(px, py, pz, a.axis[1], a.flip[1]);
      const float u = pick(px, py, pz, a.axis[2], a.flip[2]);
      const float r2 = ff * ff + ll * ll;
      bool in;
      uint32_t layer = 0;
      float key = r2;
      if constexpr (kElevation) {
        // `t >= 0` and `!(t >= 0)` as the header writes them: a NaN t takes no part
        const float h = __builtin_sqrtf(r2);
        key = r2 + u * u;
        const float t_lo = lo.x * u - lo.y * h, t_hi = hi.x * u - hi.y * h;
        in = kept && finite && r2 > 0.0f && key >= a.rmin2 && key <= a.rmax2 && t_lo >= 0.0f && !(t_hi >= 0.0f);
        up[k] = u, hz[k] = h;
      } else {
        in = kept && finite && r2 > 0.0f && r2 >= a.rmin2 && r2 <= a.rmax2 && u >= a.u_min && u < a.u_max;
        if (a.n_layers > 1) {
          const float slab = floorf((u - a.u_min) * a.inv_h);
          layer = slab >= float(a.n_layers - 1) ? uint32_t(a.n_layers - 1) : uint32_t(int(slab));   // (in: slab >= 0)
        }
      }
      const float cross0 = t0.x * ll - t0.y * ff, dot0 = t0.x * ff + t0.y * ll;
      // the half turn as a sign-bit mask, without a branch (the `if (A || (B && C)) negate` form miscompiled)
      const uint32_t turn = (uint32_t(cross0 < 0.0f) | (uint32_t(cross0 == 0.0f) & uint32_t(dot0 < 0.0f))) << 31;
      f[k] = __uint_as_float(__float_as_uint(ff) ^ turn), l[k] = __uint_as_float(__float_as_uint(ll) ^ turn);
      sector[k] = turn ? uint32_t(a.half) : 0u;
      cell[k] = in ? layer * uint32_t(a.n_sectors) : kNone;
      key_bits[k] = __float_as_uint(key);
    }
    // one broadcast LDS read of (c_j, s_j) serves the lane's records
    for (int j = 1; j < a.half; ++j) {
      const float2 b = tab[j];
#pragma unroll
      for (int k = 0; k < kMemoryPerLane; ++k) sector[k] += (b.x * l[k] - b.y * f[k]) >= 0.0f ? 1u : 0u;
    }
    if constexpr (kElevation) {
      uint32_t layer[kMemoryPerLane] = {};
      for (int i = 1; i < a.n_layers; ++i) {
        const float2 b = etab[i];
#pragma unroll
        for (int k = 0; k < kMemoryPerLane; ++k) layer[k] += (b.x * up[k] - b.y * hz[k]) >= 0.0f ? 1u : 0u;
      }
#pragma unroll
      for (int k = 0; k < kMemoryPerLane; ++k) sector[k] += layer[k] * uint32_t(a.n_sectors);   // (cell[k] is 0 or kNone here)
    }
#pragma unroll
    for (int k = 0; k < kMemoryPerLane; ++k) {
      if (cell[k] == kNone) continue;
      const uint32_t c = cell[k] + sector[k];   // (< n_cells: the layer and the sector are counts of boundaries)
      if (a.covered && a.covered[c] != 0) continue;
      const uint32_t i = uint32_t(base + k * kMemoryThreads) + tid;
      atomicMin(&carry[c], (static_cast<unsigned long long>(key_bits[k]) << 32) | i);
    }
  }
  __syncthreads();

  // ---- merge: a lane takes a cell
  for (int c = int(tid); c < a.n_cells; c += kMemoryThreads) {
    const uint32_t cnt = a.count[c], nr = a.nearest[c];
    const unsigned long long key = carry[c];
    uint4 rec = make_uint4(0u, 0u, 0u, kEmptyAge);
    float range = __uint_as_float(0x7F800000u);
    if (cnt >= a.min_count && nr < a.bound) {
      const uint4 q = a.points[size_t(nr) * size_t(a.step16)];
      const float qx = __uint_as_float(q.x), qy = __uint_as_float(q.y), qz = __uint_as_float(q.z);
      rec.x = __float_as_uint(R[0] * qx + R[1] * qy + R[2] * qz + t[0]);
      rec.y = __float_as_uint(R[3] * qx + R[4] * qy + R[5] * qz + t[1]);
      rec.z = __float_as_uint(R[6] * qx + R[7] * qy + R[8] * qz + t[2]);
      rec.w = 0u;
      const float ff = pick(q.x, q.y, q.z, a.axis[0], a.flip[0]), ll = pick(q.x, q.y, q.z, a.axis[1], a.flip[1]);
      float k2 = ff * ff + ll * ll;
      if constexpr (kElevation) {
        const float u = pick(q.x, q.y, q.z, a.axis[2], a.flip[2]);
        k2 = k2 + u * u;
      }
      range = __builtin_sqrtf(k2);
    } else if (key != ~0ull) {
      rec = src[uint32_t(key)];   // (the low word is a record of `src`: < n_cells)
      rec.w = aged(rec.w, dt);
      range = __builtin_sqrtf(__uint_as_float(uint32_t(key >> 32)));
    }
    dst[c] = rec;
    if (a.records) a.records[c] = rec;
    if (a.range) a.range[c] = range;
    if (a.age) a.age[c] = rec.w;
    if (a.distance_cm) {
      const float cm = range * 100.0f;
      a.distance_cm[c] = uint16_t(rec.w == kEmptyAge ? a.no_obstacle_cm : cm >= 65534.0f ? 65534u : uint32_t(cm));
    }
  }
  __syncthreads();
  if (tid == 0) *a.parity = par ^ 1u;
}

__global__ __launch_bounds__(256) void k_sectors_memory_reset(uint4 *buffers, int n) {
  const int i = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (i < n) buffers[i] = make_uint4(0u, 0u, 0u, kEmptyAge);
}

}  // namespace

int launch_memory_update(const MemoryLaunch &in) {
  MemoryArgs a;
  a.points = static_cast<const uint4 *>(in.points), a.count = in.count, a.nearest = in.nearest;
  a.step = static_cast<const uint32_t *>(in.step), a.covered = in.covered;
  a.table = reinterpret_cast<const float2 *>(in.table);
  a.buffers = static_cast<uint4 *>(in.buffers), a.parity = in.parity;
  a.range = in.range, a.distance_cm = in.distance_cm, a.age = in.age, a.records = static_cast<uint4 *>(in.records);
  const Plan &p = in.plan.grid;
  a.bound = in.bound, a.step16 = in.step16, a.max_age = in.plan.max_age, a.min_count = p.min_count, a.no_obstacle_cm = p.no_obstacle_cm;
  a.n_sectors = p.n_sectors, a.n_layers = p.n_layers, a.n_cells = p.n_cells, a.half = p.half;
  a.rmin2 = p.rmin2, a.rmax2 = p.rmax2, a.u_min = p.u_min, a.u_max = p.u_max, a.inv_h = p.inv_h;
  for (int i = 0; i < 3; ++i) a.axis[i] = p.axis[i], a.flip[i] = p.flip[i];
  hipStream_t s = static_cast<hipStream_t>(in.stream);
  // (the largest table, 5,760 cells with 180 + 65 boundaries, is 48,040 bytes: below the 64 KB a launch may ask for unannounced)
  if (p.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION)
    hipLaunchKernelGGL(k_sectors_memory_update<D2PC_SECTORS_LAYERS_ELEVATION>, dim3(1), dim3(kMemoryThreads), in.plan.lds_bytes, s, a);
  else
    hipLaunchKernelGGL(k_sectors_memory_update<D2PC_SECTORS_LAYERS_HEIGHT>, dim3(1), dim3(kMemoryThreads), in.plan.lds_bytes, s, a);
  return int(hipGetLastError());
}

int launch_memory_reset(void *buffers, int n_cells, void *stream) {
  const int n = 2 * n_cells;
  hipLaunchKernelGGL(k_sectors_memory_reset, dim3(unsigned((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<uint4 *>(buffers), n);
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
