// d2pc_sectors_memory.hip -- the kernels of the memory session of include/d2pc_sectors.h (gfx950).
//
// k_sectors_memory_update   ONE block of 1,024 lanes: the work is n_cells <= 5,760 records of 16 bytes, not a cloud.
//                    The carry table (one 64-bit key a cell, <= 46,080 bytes) and the azimuth / elevation tables live in
//                    LDS.  Carry: a lane takes kMemoryPerLane remembered records of buffer `parity` per pass, ages them,
//                    moves them into the frame of `points` (the transpose of R on w - t) and bins them with the
//                    statements k_sectors_reduce bins a record with (d2pc_sectors_bin.hpp: picks, gates, half turn, the steps
//                    of the boundary counts), one broadcast LDS read per boundary serving the lane's records; the key
//                    (bits(k) << 32) | record goes into the cell with one 64-bit LDS min.  Merge: a lane takes a cell; a
//                    fresh cell reads its nearest point and moves it to the world, a remembered one copies the record the
//                    key names, and the lane stores the new record to buffer 1 - parity and the outputs asked for.  The
//                    parity word is flipped on the device by the last store, so a replayed graph advances as plain calls.
//                    Vector stores only: no global atomic, nothing to clear.
// k_sectors_memory_reset    stores the empty record over both buffers.
// Every float expression is rounded once: contraction is off in this file, sqrtf is the correctly rounded one (SECTORS_FLAGS).
#include <hip/hip_runtime.h>
#include <type_traits>

#include "d2pc_sectors_bin.hpp"
#include "d2pc_sectors_memory_plan.hpp"

namespace d2pc {
namespace sectors {
namespace {

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
  uint32_t bound, step16, max_age;
  GridArgs grid;
};

// a' = min(a + dt, 0xFFFFFFFE) without wrap
__device__ __forceinline__ uint32_t aged(uint32_t a, uint32_t dt) {
  const unsigned long long s = static_cast<unsigned long long>(a) + dt;
  return s > kOldestAge ? kOldestAge : uint32_t(s);
}

template <int kKind>
__global__ __launch_bounds__(kMemoryThreads) void k_sectors_memory_update(const MemoryArgs a) {
#pragma clang fp contract(off)
  constexpr bool kElevation = kKind == D2PC_SECTORS_LAYERS_ELEVATION;
  const GridArgs g = a.grid;
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned long long *carry = reinterpret_cast<unsigned long long *>(lds);
  float2 *tab = reinterpret_cast<float2 *>(carry + g.n_cells);   // then n_layers + 1 x (ce, se), behind the azimuth table
  const uint32_t tid = threadIdx.x;
  for (int i = int(tid); i < g.n_cells; i += kMemoryThreads) carry[i] = ~0ull;
  for (int j = int(tid); j < g.half + (kElevation ? g.n_layers + 1 : 0); j += kMemoryThreads) tab[j] = a.table[j];
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = __uint_as_float(a.step[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = __uint_as_float(a.step[9 + i]);
  const uint32_t dt = a.step[12];
  const uint32_t par = *a.parity & 1u;   // (read by every lane before the barriers; lane 0 stores it behind the last one)
  const uint4 *src = a.buffers + size_t(par) * size_t(g.n_cells);
  uint4 *dst = a.buffers + size_t(par ^ 1u) * size_t(g.n_cells);
  __syncthreads();

  // ---- carry: the remembered records of `src` into the cells they fall into under the new pose
  for (int base = 0; base < g.n_cells; base += kMemoryThreads * kMemoryPerLane) {
    if (base + int(tid & ~63u) >= g.n_cells) continue;   // wave-uniform: none of this wave's records exists
    float f[kMemoryPerLane], l[kMemoryPerLane], up[kMemoryPerLane], hz[kMemoryPerLane];
    uint32_t cell[kMemoryPerLane], key_bits[kMemoryPerLane], sector[kMemoryPerLane], layer[kMemoryPerLane] = {};
    const float2 t0 = tab[0], lo = tab[kElevation ? g.half : 0], hi = tab[kElevation ? g.half + g.n_layers : 0];
    uint4 p[kMemoryPerLane];   // the records in the frame of `points`, and whether each is still remembered
    bool kept[kMemoryPerLane];
#pragma unroll
    for (int k = 0; k < kMemoryPerLane; ++k) {
      const int i = base + k * kMemoryThreads + int(tid);
      uint4 w = make_uint4(0u, 0u, 0u, kEmptyAge);
      if (i < g.n_cells) w = src[i];
      kept[k] = w.w != kEmptyAge && aged(w.w, dt) <= a.max_age;
      const float dx = __uint_as_float(w.x) - t[0], dy = __uint_as_float(w.y) - t[1], dz = __uint_as_float(w.z) - t[2];
      p[k] = make_uint4(__float_as_uint(R[0] * dx + R[3] * dy + R[6] * dz), __float_as_uint(R[1] * dx + R[4] * dy + R[7] * dz),
                        __float_as_uint(R[2] * dx + R[5] * dy + R[8] * dz), 0u);
    }
    // k_sectors_reduce's own step (d2pc_sectors_bin.hpp).  The record goes in as measured: by reference the
    // elevation kernel is 1 % faster than by value at 87 VGPRs, the height kernel would hold 84 where by value it holds 67
    using Record = std::conditional_t<kElevation, const uint4 &, uint4>;
#pragma unroll
    for (int k = 0; k < kMemoryPerLane; ++k) {
      const Binned b = bin_record<kElevation, Record>(g, t0, lo, hi, p[k], kept[k]);
      f[k] = b.f, l[k] = b.l, up[k] = b.up, hz[k] = b.hz, cell[k] = b.cell, key_bits[k] = b.key_bits, sector[k] = b.sector;
    }
    for (int j = 1; j < g.half; ++j) {
      const float2 bd = tab[j];
#pragma unroll
      for (int k = 0; k < kMemoryPerLane; ++k) sector[k] += behind(bd, l[k], f[k]);
    }
    for (int i = 1; kElevation && i < g.n_layers; ++i) {
      const float2 bd = tab[g.half + i];
#pragma unroll
      for (int k = 0; k < kMemoryPerLane; ++k) layer[k] += behind(bd, up[k], hz[k]);
    }
#pragma unroll
    for (int k = 0; k < kMemoryPerLane; ++k) {
      const uint32_t c = cell_of(g, cell[k], sector[k], layer[k]);
      if (c == kNone) continue;
      if (a.covered && a.covered[c] != 0) continue;
      const uint32_t i = uint32_t(base + k * kMemoryThreads) + tid;
      atomicMin(&carry[c], (static_cast<unsigned long long>(key_bits[k]) << 32) | i);
    }
  }
  __syncthreads();

  // ---- merge: a lane takes a cell
  for (int c = int(tid); c < g.n_cells; c += kMemoryThreads) {
    const uint32_t cnt = a.count[c], nr = a.nearest[c];
    const unsigned long long key = carry[c];
    uint4 rec = make_uint4(0u, 0u, 0u, kEmptyAge);
    float range = __uint_as_float(0x7F800000u);
    if (cnt >= g.min_count && nr < a.bound) {
      const uint4 q = a.points[size_t(nr) * size_t(a.step16)];
      const float qx = __uint_as_float(q.x), qy = __uint_as_float(q.y), qz = __uint_as_float(q.z);
      rec.x = __float_as_uint(R[0] * qx + R[1] * qy + R[2] * qz + t[0]);
      rec.y = __float_as_uint(R[3] * qx + R[4] * qy + R[5] * qz + t[1]);
      rec.z = __float_as_uint(R[6] * qx + R[7] * qy + R[8] * qz + t[2]);
      rec.w = 0u;
      const float ff = pick<uint4>(q, g.axis[0], g.flip[0]), ll = pick<uint4>(q, g.axis[1], g.flip[1]), u = pick<uint4>(q, g.axis[2], g.flip[2]);
      const float r2 = ff * ff + ll * ll;
      range = __builtin_sqrtf(kElevation ? r2 + u * u : r2);   // k(q): the very bits the sectors call wrote
    } else if (key != ~0ull) {
      rec = src[uint32_t(key)];   // (the low word is a record of `src`: < n_cells)
      rec.w = aged(rec.w, dt);
      range = range_of_key(key);
    }
    dst[c] = rec;
    if (a.records) a.records[c] = rec;
    if (a.range) a.range[c] = range;
    if (a.age) a.age[c] = rec.w;
    if (a.distance_cm) a.distance_cm[c] = distance_cm_of(g, range, rec.w == kEmptyAge);
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
  a.bound = in.bound, a.step16 = in.step16, a.max_age = in.plan.max_age;
  a.grid = grid_args(in.plan.grid);
  // (the largest table, 5,760 cells with 180 + 65 boundaries, is 48,040 bytes: below the 64 KB a launch may ask for unannounced)
  void *args[] = {&a};
  const void *kernel = in.plan.grid.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION   // the one place that turns a layer kind into this kernel
                           ? reinterpret_cast<const void *>(&k_sectors_memory_update<D2PC_SECTORS_LAYERS_ELEVATION>)
                           : reinterpret_cast<const void *>(&k_sectors_memory_update<D2PC_SECTORS_LAYERS_HEIGHT>);
  (void)hipLaunchKernel(kernel, dim3(1), dim3(kMemoryThreads), args, in.plan.lds_bytes, static_cast<hipStream_t>(in.stream));
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
