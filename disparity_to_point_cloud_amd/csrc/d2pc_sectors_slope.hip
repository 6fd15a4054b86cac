// d2pc_sectors_slope.hip -- the three kernels of the slope session of include/d2pc_sectors.h (gfx950).
//
// k_slope_reduce     k_ground_reduce's walk (d2pc_sectors_device.hpp: a share is 1,024 records of one cloud, four 16-byte
//                    loads in flight per lane; a 32-byte record is the load of its first half) and its binning, then step 9
//                    of the SLOPE block.  Each block keeps a private table of the cells in dynamic LDS, plane after plane:
//                    nine 64-bit words (sum, sum2, su, sw, suu, suw, sww, suk, swk) and the count, 76 bytes per cell, and
//                    every lane issues its own ten LDS adds, the plain form that won DESIGN.md 8g's A/B.  All nine sums
//                    stay 64 bits wide: a call may hold 2^32 - 1 positions and a block may walk all of them, so no plan
//                    bounds a block's partial sums below 32 bits.  At the end the block stores its table to its own slab
//                    with plain vector stores: no global atomic, nothing to clear, no protocol between blocks.
// k_slope_merge      sums over the slabs of the blocks that ran, 16 cells x 16 slices of the slabs per block, a tree through
//                    LDS over the slices, then the integer pre-steps and the fit in double, one cell a lane, and the
//                    per-cell outputs the caller asked for and the 14 bytes per cell the sites read.
// k_slope_sites      ONE block of 1,024 lanes that calls ground_site_stage (d2pc_sectors_ground_sites.hpp) on level_q,
//                    resid_q2 and the slope's flat, and then stores the number of fitted cells over summary word 3.
// The fit and the site launch's body are d2pc_sectors_slope_fit.hpp's: the relief's kernels call the same.
// Every accumulated value is an integer and the fit is one fixed sequence of double operations per cell: the result is the
// same bytes whatever order lanes, waves and blocks arrive in.  Every float and double expression of the specification is
// rounded once: contraction is off in this file.
#include <hip/hip_runtime.h>

#include "d2pc_sectors_slope_fit.hpp"

namespace d2pc {
namespace sectors {
namespace {

struct SlopeArgs {   // SlopeLaunch without its host-only members
  CloudWalk walk;
  const float *step;
  const uint8_t *allowed;
  unsigned long long *slabs;
  uint32_t *hand_on;
  uint32_t *count;
  unsigned long long *sum, *sum2, *moments;
  uint32_t *slope_a, *slope_b, *level_q, *resid_q2;
  uint8_t *flat, *site;
  unsigned long long *candidates;
  uint32_t *summary;
  int blocks, n_candidates;
  GroundSiteGrid grid;
  int axis_a, axis_b, axis_h;
  uint32_t flip_a, flip_b, flip_h;
  float inv_c, inv_q, sub;
  int sub_less_1;
  SlopeFit fit;   // (d2pc_sectors_slope_fit.hpp)
};

// the block's slab: the nine 64-bit planes of n_cells each, then the counts
__device__ __forceinline__ unsigned long long *slab_of(const SlopeArgs &a, int block) {
  return a.slabs + size_t(block) * (size_t(kSlopeWords) * size_t(a.grid.n_cells) + (size_t(a.grid.n_cells) + 1u) / 2u);   // (SlopePlan::block_bytes, in 64-bit words)
}

__device__ __forceinline__ unsigned long long wide(int v) { return static_cast<unsigned long long>(static_cast<long long>(v)); }

// one record of a lane into the block's table: the lane's own ten LDS adds (the 64-bit add is native).  k is the height in
// quanta, |k| <= 32767; u and w are odd, |u|, |w| <= 15: every term is below 2^19 in magnitude, k * k below 2^30
__device__ __forceinline__ void merge(unsigned long long *tab, uint32_t *cnt, int n_cells, uint32_t cell, int k, int u, int w) {
  if (cell == kNone) return;
  unsigned long long *t = tab + cell;
  atomicAdd(t, wide(k));
  atomicAdd(t + n_cells, wide(k * k));
  atomicAdd(t + 2 * n_cells, wide(u));
  atomicAdd(t + 3 * n_cells, wide(w));
  atomicAdd(t + 4 * n_cells, wide(u * u));
  atomicAdd(t + 5 * n_cells, wide(u * w));
  atomicAdd(t + 6 * n_cells, wide(w * w));
  atomicAdd(t + 7 * n_cells, wide(u * k));
  atomicAdd(t + 8 * n_cells, wide(w * k));
  atomicAdd(&cnt[cell], 1u);
}

__device__ __forceinline__ float pick(int axis, uint32_t flip, float x, float y, float z) {
  const float v = axis == 0 ? x : (axis == 1 ? y : z);
  return __uint_as_float(__float_as_uint(v) ^ flip);   // (a negation is exact)
}

__global__ __launch_bounds__(kThreads) void k_slope_reduce(const SlopeArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char lds[];
  const int n_cells = a.grid.n_cells;
  unsigned long long *tab = reinterpret_cast<unsigned long long *>(lds);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(tab + kSlopeWords * n_cells);
  const uint32_t tid = threadIdx.x;
  for (int i = int(tid); i < kSlopeWords * n_cells; i += kThreads) tab[i] = 0ull;
  for (int i = int(tid); i < n_cells; i += kThreads) cnt[i] = 0u;
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
    int q[kPerLane], u[kPerLane], w[kPerLane];
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
      const float fla = floorf(va), flb = floorf(vb);
      const int ia = int(fla), ib = int(flb);
      cell[k] = part ? uint32_t(ib * a.grid.n_a + ia) : kNone;
      q[k] = part ? int(rintf(v)) : 0;
      // step 9: the position in the cell, in half sub-steps from its centre (both float operations are exact)
      u[k] = part ? 2 * int(floorf((va - fla) * a.sub)) - a.sub_less_1 : 0;
      w[k] = part ? 2 * int(floorf((vb - flb) * a.sub)) - a.sub_less_1 : 0;
    }
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) merge(tab, cnt, n_cells, cell[k], q[k], u[k], w[k]);
  }

  __syncthreads();
  unsigned long long *slab = slab_of(a, int(blockIdx.x));
  uint32_t *slab_c = reinterpret_cast<uint32_t *>(slab + size_t(kSlopeWords) * size_t(n_cells));
  for (int i = int(tid); i < kSlopeWords * n_cells; i += kThreads) slab[i] = tab[i];
  for (int i = int(tid); i < n_cells; i += kThreads) slab_c[i] = cnt[i];
}

__global__ __launch_bounds__(kThreads) void k_slope_merge(const SlopeArgs a) {
  __shared__ unsigned long long sw[kSlopeWords][kThreads];
  __shared__ uint32_t sc[kThreads];
  const int tid = int(threadIdx.x), slice = tid / kGroundMergeCells;
  const int cell = int(blockIdx.x) * kGroundMergeCells + tid % kGroundMergeCells;
  const int n_cells = a.grid.n_cells;
  unsigned long long s[kSlopeWords] = {};
  uint32_t cnt = 0;
  if (cell < n_cells) {
    for (int b = slice; b < a.blocks; b += kGroundMergeSlices) {
      const unsigned long long *slab = slab_of(a, b);
#pragma unroll
      for (int p = 0; p < kSlopeWords; ++p) s[p] += slab[p * n_cells + cell];
      cnt += reinterpret_cast<const uint32_t *>(slab + size_t(kSlopeWords) * size_t(n_cells))[cell];
    }
  }
#pragma unroll
  for (int p = 0; p < kSlopeWords; ++p) sw[p][tid] = s[p];
  sc[tid] = cnt;
  for (int h = kGroundMergeSlices / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (slice < h) {
#pragma unroll
      for (int p = 0; p < kSlopeWords; ++p) s[p] += sw[p][tid + h * kGroundMergeCells], sw[p][tid] = s[p];
      cnt += sc[tid + h * kGroundMergeCells], sc[tid] = cnt;
    }
  }
  if (slice != 0 || cell >= n_cells) return;
  const SlopeCell o = slope_cell_fit(a.fit, cnt, s);   // (d2pc_sectors_slope_fit.hpp)
  if (a.count) a.count[cell] = cnt;
  if (a.sum) a.sum[cell] = s[0];
  if (a.sum2) a.sum2[cell] = s[1];
  if (a.moments) {
#pragma unroll
    for (int p = 0; p < D2PC_SECTORS_SLOPE_MOMENTS; ++p) a.moments[size_t(p) * size_t(n_cells) + cell] = s[2 + p];
  }
  if (a.slope_a) a.slope_a[cell] = o.slope_a;
  if (a.slope_b) a.slope_b[cell] = o.slope_b;
  if (a.level_q) a.level_q[cell] = o.level_q;
  if (a.resid_q2) a.resid_q2[cell] = o.resid_q2;
  if (a.flat) a.flat[cell] = o.flat;
  slope_hand_on(a.hand_on, n_cells, cell, cnt, o);
}

__global__ __launch_bounds__(kGroundSiteThreads) void k_slope_sites(const SlopeArgs a) {
  __shared__ GroundSiteLds lds;
  __shared__ uint32_t fit_slot[kGroundSiteWaves];
  GroundSiteStage st;
  st.grid = a.grid, st.n_candidates = a.n_candidates;
  st.goal_i = reinterpret_cast<const uint32_t *>(a.step)[15], st.goal_j = reinterpret_cast<const uint32_t *>(a.step)[16];
  st.allowed = a.allowed, st.site = a.site, st.candidates = a.candidates, st.summary = a.summary;
  slope_sites_from_hand_on(a.hand_on, st, lds, fit_slot);   // (d2pc_sectors_slope_fit.hpp)
}

}  // namespace

int prepare_slope_kernels(const SlopePlan &p) {
  // beyond 64 KB of dynamic LDS the runtime wants to be told (46 x 46 cells need 160,816 bytes)
  if (p.lds_bytes <= 64u * 1024u) return int(hipSuccess);
  return int(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_slope_reduce), hipFuncAttributeMaxDynamicSharedMemorySize, int(p.lds_bytes)));
}

int launch_slope(const SlopeLaunch &in) {
  SlopeArgs a;
  a.walk = in.walk, a.step = static_cast<const float *>(in.step);
  a.allowed = in.allowed;
  a.slabs = static_cast<unsigned long long *>(in.slabs), a.hand_on = static_cast<uint32_t *>(in.hand_on);
  a.count = in.count, a.sum = reinterpret_cast<unsigned long long *>(in.sum), a.sum2 = reinterpret_cast<unsigned long long *>(in.sum2);
  a.moments = reinterpret_cast<unsigned long long *>(in.moments);
  a.slope_a = reinterpret_cast<uint32_t *>(in.slope_a), a.slope_b = reinterpret_cast<uint32_t *>(in.slope_b);
  a.level_q = reinterpret_cast<uint32_t *>(in.level_q), a.resid_q2 = in.resid_q2, a.flat = in.flat, a.site = in.site;
  a.candidates = static_cast<unsigned long long *>(in.candidates), a.summary = in.summary;
  a.n_candidates = in.candidates ? in.n_candidates : 0;
  a.blocks = in.blocks;
  const GroundPlan &g = in.plan.ground;
  a.grid = ground_site_grid(g);
  a.axis_a = g.axis[0], a.axis_b = g.axis[1], a.axis_h = g.axis[2];
  a.flip_a = g.flip[0], a.flip_b = g.flip[1], a.flip_h = g.flip[2];
  a.inv_c = g.inv_c, a.inv_q = g.inv_q;
  a.sub = float(in.plan.sub), a.sub_less_1 = in.plan.sub - 1;
  a.fit = slope_fit_of(in.plan);
  hipStream_t s = static_cast<hipStream_t>(in.stream);
  void *args[] = {&a};
  (void)hipLaunchKernel(reinterpret_cast<const void *>(&k_slope_reduce), dim3(unsigned(in.blocks)), dim3(kThreads), args, in.plan.lds_bytes, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return int(e);
  hipLaunchKernelGGL(k_slope_merge, dim3(unsigned((g.n_cells + kGroundMergeCells - 1) / kGroundMergeCells)), dim3(kThreads), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess || !(in.site || in.candidates || in.summary)) return int(e);
  hipLaunchKernelGGL(k_slope_sites, dim3(1), dim3(kGroundSiteThreads), 0, s, a);
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
