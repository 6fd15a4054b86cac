// d2pc_sectors_ground.hip -- the three kernels of the ground session of include/d2pc_sectors.h (gfx950).
//
// k_ground_reduce    min(the session's blocks, the call's shares) blocks of 256 lanes; block b walks shares b, b + blocks, ...
//                    of the call's records as k_sectors_reduce does (a share is 1,024 records of one cloud, four 16-byte
//                    loads in flight per lane; a 32-byte record is the load of its first half).  About a dozen VALU
//                    operations bin a record, so the LDS atomics are what it costs.  Each block keeps a private table of
//                    the cells in dynamic LDS: sum (64-bit), sum2 (64-bit), count, 20 bytes per cell, and every lane issues
//                    its own three LDS adds (the 64-bit add is native).  The other form, an in-wave pre-reduction of the
//                    lanes that share a cell, lost in seven rows of eight and left the sources: DESIGN.md 8g.
//                    At the end the block stores its table to its own slab with plain vector stores: no global atomic,
//                    nothing to clear, no protocol between blocks.
// k_ground_merge     sums over the slabs of the blocks that ran, 16 cells x 16 slices of the slabs per block (a row of 16
//                    cells is a whole 128-byte line of the 64-bit sums), a tree through LDS over the slices, then the six
//                    per-cell outputs the caller asked for and the 13 bytes per cell the sites read.
// k_ground_sites     ONE block of 1,024 lanes, four cells a lane at the most: mean_q and flat into LDS, the direct
//                    (2W + 1)^2 walk, cost and key in registers, the K smallest keys with the steer's rounds (DPP minima of
//                    cost then cell, one 64-bit LDS min into the round's own word, one barrier a round), the summary from
//                    wave reductions.  It reads what the merge wrote behind a kernel boundary: no global atomic.
//                    The stage itself, and the merge's per-cell formula, are d2pc_sectors_ground_sites.hpp's: the terrain's
//                    kernel (d2pc_sectors_terrain.hip) runs the same two on a window's sums.
// Every accumulated value is an integer: the result is the same bytes whatever order lanes, waves and blocks arrive in.
// Every float expression of the specification is rounded once: contraction is off in this file.
#include <hip/hip_runtime.h>

#include "d2pc_sectors_ground_sites.hpp"

namespace d2pc {
namespace sectors {
namespace {

struct GroundArgs {   // GroundLaunch without its host-only members
  CloudWalk walk;
  const float *step;
  const uint8_t *allowed;
  unsigned long long *slabs;
  uint32_t *hand_on;
  uint32_t *count;
  unsigned long long *sum, *sum2;
  uint32_t *mean_q, *spread_q2;
  uint8_t *flat, *site;
  unsigned long long *candidates;
  uint32_t *summary;
  int blocks, n_candidates;
  GroundSiteGrid grid;
  int axis_a, axis_b, axis_h;
  uint32_t flip_a, flip_b, flip_h;
  float inv_c, inv_q;
  uint32_t min_count, max_spread_q2;
};

// the block's slab: sum and sum2 as 64-bit words of n_cells each, then the counts
__device__ __forceinline__ unsigned long long *slab_of(const GroundArgs &a, int block) {
  return a.slabs + size_t(block) * (2u * size_t(a.grid.n_cells) + (size_t(a.grid.n_cells) + 1u) / 2u);   // (GroundPlan::block_bytes, in 64-bit words)
}

// one record of a lane into the block's table: the lane's own three LDS adds; k is the height in quanta, |k| <= 32767
__device__ __forceinline__ void merge(unsigned long long *sum, unsigned long long *sum2, uint32_t *cnt, uint32_t cell, int k) {
  if (cell == kNone) return;
  atomicAdd(&sum[cell], static_cast<unsigned long long>(static_cast<long long>(k)));
  atomicAdd(&sum2[cell], static_cast<unsigned long long>(uint32_t(k * k)));   // < 2^30
  atomicAdd(&cnt[cell], 1u);
}

__device__ __forceinline__ float pick(int axis, uint32_t flip, float x, float y, float z) {
  const float v = axis == 0 ? x : (axis == 1 ? y : z);
  return __uint_as_float(__float_as_uint(v) ^ flip);   // (a negation is exact)
}

__global__ __launch_bounds__(kThreads) void k_ground_reduce(const GroundArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned long long *sum = reinterpret_cast<unsigned long long *>(lds);
  unsigned long long *sum2 = sum + a.grid.n_cells;
  uint32_t *cnt = reinterpret_cast<uint32_t *>(sum2 + a.grid.n_cells);
  const uint32_t tid = threadIdx.x;
  for (int i = int(tid); i < a.grid.n_cells; i += kThreads) sum[i] = 0ull, sum2[i] = 0ull, cnt[i] = 0u;
  // the step: the same 15 words in every lane
  const float r0 = a.step[0], r1 = a.step[1], r2 = a.step[2], r3 = a.step[3], r4 = a.step[4], r5 = a.step[5], r6 = a.step[6],
              r7 = a.step[7], r8 = a.step[8], tx = a.step[9], ty = a.step[10], tz = a.step[11], a0 = a.step[12], b0 = a.step[13],
              h0 = a.step[14];
  const float na = float(a.grid.n_a), nb = float(a.grid.n_b);
  __syncthreads();

  for (uint64_t share = blockIdx.x; share < a.walk.shares; share += uint64_t(a.blocks)) {
    ShareAt at;
    if (!find_share(a.walk, share, &at)) continue;   // (d2pc_sectors_device.hpp)
    uint4 rec[kPerLane];
    bool have[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) rec[k] = share_record(a.walk, at, tid, k, &have[k]);
    uint32_t cell[kPerLane];
    int q[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const bool finite = (rec[k].x & 0x7F800000u) != 0x7F800000u && (rec[k].y & 0x7F800000u) != 0x7F800000u &&
                          (rec[k].z & 0x7F800000u) != 0x7F800000u;
      const float x = __uint_as_float(rec[k].x), y = __uint_as_float(rec[k].y), z = __uint_as_float(rec[k].z);
      const float wx = ((r0 * x + r1 * y) + r2 * z) + tx;
      const float wy = ((r3 * x + r4 * y) + r5 * z) + ty;
      const float wz = ((r6 * x + r7 * y) + r8 * z) + tz;
      const float pa = pick(a.axis_a, a.flip_a, wx, wy, wz), pb = pick(a.axis_b, a.flip_b, wx, wy, wz);
      const float ph = pick(a.axis_h, a.flip_h, wx, wy, wz);
      const float va = (pa - a0) * a.inv_c, vb = (pb - b0) * a.inv_c, v = (ph - h0) * a.inv_q;
      const bool part = have[k] && finite && va >= 0.0f && va < na && vb >= 0.0f && vb < nb && v >= -32767.0f && v <= 32767.0f;
      const int ia = int(floorf(va)), ib = int(floorf(vb));
      cell[k] = part ? uint32_t(ib * a.grid.n_a + ia) : kNone;
      q[k] = part ? int(rintf(v)) : 0;
    }
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) merge(sum, sum2, cnt, cell[k], q[k]);
  }

  __syncthreads();
  unsigned long long *slab = slab_of(a, int(blockIdx.x));
  uint32_t *slab_c = reinterpret_cast<uint32_t *>(slab + 2 * size_t(a.grid.n_cells));
  for (int i = int(tid); i < a.grid.n_cells; i += kThreads) slab[i] = sum[i], slab[a.grid.n_cells + i] = sum2[i], slab_c[i] = cnt[i];
}

__global__ __launch_bounds__(kThreads) void k_ground_merge(const GroundArgs a) {
  __shared__ unsigned long long s1[kThreads], s2[kThreads];
  __shared__ uint32_t sc[kThreads];
  const int tid = int(threadIdx.x), slice = tid / kGroundMergeCells;
  const int cell = int(blockIdx.x) * kGroundMergeCells + tid % kGroundMergeCells;
  const int n_cells = a.grid.n_cells;
  unsigned long long sum = 0, sum2 = 0;
  uint32_t cnt = 0;
  if (cell < n_cells) {
#pragma unroll 4
    for (int b = slice; b < a.blocks; b += kGroundMergeSlices) {
      const unsigned long long *slab = slab_of(a, b);
      sum += slab[cell], sum2 += slab[n_cells + cell];
      cnt += reinterpret_cast<const uint32_t *>(slab + 2 * size_t(n_cells))[cell];
    }
  }
  s1[tid] = sum, s2[tid] = sum2, sc[tid] = cnt;
  for (int s = kGroundMergeSlices / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (slice < s) {
      sum += s1[tid + s * kGroundMergeCells], sum2 += s2[tid + s * kGroundMergeCells], cnt += sc[tid + s * kGroundMergeCells];
      s1[tid] = sum, s2[tid] = sum2, sc[tid] = cnt;
    }
  }
  if (slice != 0 || cell >= n_cells) return;
  uint32_t mean, spread;
  ground_cell_formula(cnt, sum, sum2, &mean, &spread);   // (d2pc_sectors_ground_sites.hpp: the terrain's formula too)
  const uint8_t flat = cnt >= a.min_count && spread <= a.max_spread_q2 ? 1 : 0;   // (min_count >= 1: an empty cell is never flat)
  if (a.count) a.count[cell] = cnt;
  if (a.sum) a.sum[cell] = sum;
  if (a.sum2) a.sum2[cell] = sum2;
  if (a.mean_q) a.mean_q[cell] = mean;
  if (a.spread_q2) a.spread_q2[cell] = spread;
  if (a.flat) a.flat[cell] = flat;
  a.hand_on[cell] = cnt, a.hand_on[n_cells + cell] = mean, a.hand_on[2 * n_cells + cell] = spread;
  reinterpret_cast<uint8_t *>(a.hand_on + 3 * size_t(n_cells))[cell] = flat;
}

__global__ __launch_bounds__(kGroundSiteThreads) void k_ground_sites(const GroundArgs a) {
  __shared__ GroundSiteLds lds;
  const int tid = int(threadIdx.x);
  const int n_cells = a.grid.n_cells;
  const uint8_t *flat_g = reinterpret_cast<const uint8_t *>(a.hand_on + 3 * size_t(n_cells));
  uint32_t points = 0, n_flat = 0;
  uint32_t spread[kGroundPerLane] = {};
#pragma unroll
  for (int k = 0; k < kGroundPerLane; ++k) {
    const int c = tid + k * kGroundSiteThreads;
    if (c >= n_cells) continue;
    const uint8_t f = flat_g[c];
    points += a.hand_on[c], n_flat += f;
    lds.mean_q[c] = int(a.hand_on[n_cells + c]), lds.flat[c] = f;
    spread[k] = a.hand_on[2 * n_cells + c];
  }
  GroundSiteStage st;
  st.grid = a.grid, st.n_candidates = a.n_candidates;
  st.goal_i = reinterpret_cast<const uint32_t *>(a.step)[15], st.goal_j = reinterpret_cast<const uint32_t *>(a.step)[16];
  st.allowed = a.allowed, st.site = a.site, st.candidates = a.candidates, st.summary = a.summary;
  ground_site_stage(st, lds, spread, points, n_flat);   // (d2pc_sectors_ground_sites.hpp: the terrain's site stage too)
}

}  // namespace

int prepare_ground_kernels(const GroundPlan &p) {
  // beyond 64 KB of dynamic LDS the runtime wants to be told (64 x 64 cells need 81,920 bytes)
  if (p.lds_bytes <= 64u * 1024u) return int(hipSuccess);
  return int(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_ground_reduce), hipFuncAttributeMaxDynamicSharedMemorySize, int(p.lds_bytes)));
}

int launch_ground(const GroundLaunch &in) {
  GroundArgs a;
  a.walk = in.walk, a.step = static_cast<const float *>(in.step);
  a.allowed = in.allowed;
  a.slabs = static_cast<unsigned long long *>(in.slabs), a.hand_on = static_cast<uint32_t *>(in.hand_on);
  a.count = in.count, a.sum = reinterpret_cast<unsigned long long *>(in.sum), a.sum2 = reinterpret_cast<unsigned long long *>(in.sum2);
  a.mean_q = reinterpret_cast<uint32_t *>(in.mean_q), a.spread_q2 = in.spread_q2, a.flat = in.flat, a.site = in.site;
  a.candidates = static_cast<unsigned long long *>(in.candidates), a.summary = in.summary;
  a.n_candidates = in.candidates ? in.n_candidates : 0;
  a.blocks = in.blocks;
  const GroundPlan &p = in.plan;
  a.grid = ground_site_grid(p);
  a.axis_a = p.axis[0], a.axis_b = p.axis[1], a.axis_h = p.axis[2];
  a.flip_a = p.flip[0], a.flip_b = p.flip[1], a.flip_h = p.flip[2];
  a.inv_c = p.inv_c, a.inv_q = p.inv_q;
  a.min_count = p.min_count, a.max_spread_q2 = p.max_spread_q2;
  hipStream_t s = static_cast<hipStream_t>(in.stream);
  void *args[] = {&a};
  (void)hipLaunchKernel(reinterpret_cast<const void *>(&k_ground_reduce), dim3(unsigned(in.blocks)), dim3(kThreads), args, p.lds_bytes, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return int(e);
  hipLaunchKernelGGL(k_ground_merge, dim3(unsigned((p.n_cells + kGroundMergeCells - 1) / kGroundMergeCells)), dim3(kThreads), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess || !(in.site || in.candidates || in.summary)) return int(e);
  hipLaunchKernelGGL(k_ground_sites, dim3(1), dim3(kGroundSiteThreads), 0, s, a);
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
