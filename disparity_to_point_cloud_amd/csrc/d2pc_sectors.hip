// d2pc_sectors.hip -- the two kernels of include/d2pc_sectors.h (gfx950).
//
// k_sectors_reduce   a fixed grid of blocks; block b walks shares b, b + blocks, ... of the call's records (a share is
//                    1,024 records of one cloud: 4 per lane, four 16-byte loads in flight per lane; a 32-byte record is
//                    the 16-byte load of its first half).  Each block keeps a private table of the cells (64-bit key,
//                    32-bit count) and the boundary table in LDS.  Neighbouring records of a row-major cloud fall into
//                    the same cell, so a wave first reduces inside itself: the cell of the first live lane is elected,
//                    the lanes that match it take a wave minimum of the key (two 32-bit DPP reductions: r2, then the
//                    position among equal r2) and a population count, ONE lane issues one 64-bit LDS min and one LDS add.
//                    Two such rounds; lanes still live after them issue their own LDS atomics.  The rounds are a
//                    launch-uniform number, 2 for grids of at most kWaveRoundsMaxCells cells and 0 (per-lane LDS atomics
//                    alone) for larger ones, as measured (profiles/sectors_ab.txt): a wave of neighbouring
//                    records spans one or two 5-degree sectors but half a dozen 1-degree ones times the layers, and
//                    electing cells that few lanes share costs more than the atomics it saves.
//                    -DD2PC_SECTORS_FORCE_ROUNDS=0 / =2 build the two arms (tools/sectors_bench.py --ab).
//                    At the end the block stores its table to its own slab with plain vector stores: no global atomic,
//                    nothing to clear, no protocol between blocks.
//                    A template on the layer kind.  <HEIGHT> is the statements above and nothing else.  <ELEVATION> keeps
//                    the elevation table (ce_i, se_i) in LDS behind the azimuth table, gates on the Euclidean d2 and on the
//                    band's two boundaries, counts the interior boundaries below the point in a second loop of the azimuth
//                    loop's shape (one broadcast LDS read per boundary serves the lane's four records) and keys on d2.
// k_sectors_finish   min / sum over the slabs, coalesced across cells (8 cells x 32 slices of the slabs per block, a
//                    tree through LDS over the slices), then the outputs the caller asked for.
// Keys are integers and counts are sums of integers: the result is the same bytes whatever order lanes, waves and
// blocks arrive in.  Every float expression of the specification is rounded once: contraction is off in this file.
#include <hip/hip_runtime.h>

#include "d2pc_sectors_plan.hpp"


namespace d2pc {
namespace sectors {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;   // a lane without a participating point
[[maybe_unused]] constexpr int kWaveRounds = 2;   // elected cells per wave and record slot ...
[[maybe_unused]] constexpr int kWaveRoundsMaxCells = 72;   // ... for grids up to this many cells; none beyond
constexpr int kFinishCells = 8, kFinishSlices = 32;
static_assert(kFinishCells * kFinishSlices == kThreads, "the finishing block is cells x slices");

struct Args {   // Launch without its host-only members
  const uint4 *points;
  const uint32_t *counts;
  const float2 *table;
  uint64_t *slab_keys;
  uint32_t *slab_counts;
  float *range;
  uint32_t *count, *nearest;
  uint16_t *distance_cm;
  uint64_t stride, shares;
  uint32_t shares_per_cloud, cloud_points, n_clouds, step16;
  int n_sectors, n_layers, n_cells, half, blocks, rounds;
  float rmin2, rmax2, u_min, u_max, inv_h;
  int axis[3];
  uint32_t flip[3];
  uint32_t min_count, no_obstacle_cm;
};

// the minimum over the wave's 64 lanes, in every lane; all 64 lanes are active at every call (the callers' control
// flow is uniform).  row_shr 1, 2, 4, 8 scan a row of 16; row_bcast:15 / :31 carry the rows' totals on: lane 63 holds all
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
#define D2PC_DPP_MIN(ctrl, rows) \
  v = min(v, uint32_t(__builtin_amdgcn_update_dpp(int(kNone), int(v), ctrl, rows, 0xf, false)))
  D2PC_DPP_MIN(0x111, 0xf);
  D2PC_DPP_MIN(0x112, 0xf);
  D2PC_DPP_MIN(0x114, 0xf);
  D2PC_DPP_MIN(0x118, 0xf);
  D2PC_DPP_MIN(0x142, 0xa);
  D2PC_DPP_MIN(0x143, 0xc);
#undef D2PC_DPP_MIN
  return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}

__device__ __forceinline__ float pick(const uint4 &p, int axis, uint32_t flip) {
  return __uint_as_float((axis == 0 ? p.x : axis == 1 ? p.y : p.z) ^ flip);
}

// one record slot of the wave into the block's table
__device__ __forceinline__ void merge(unsigned long long *keys, uint32_t *cnts, int rounds, uint32_t cell, uint32_t r2_bits,
                                      uint32_t pos) {
  bool live = cell != kNone;
  const uint32_t lane = __lane_id();
  for (int round = 0; round < rounds; ++round) {
    const unsigned long long any = __ballot(live);
    if (any == 0) break;
    const int leader = __ffsll(any) - 1;
    const uint32_t elected = uint32_t(__builtin_amdgcn_readlane(int(cell), leader));
    const bool mine = live && cell == elected;
    const uint32_t n = uint32_t(__popcll(__ballot(mine)));
    const uint32_t r2_min = wave_umin(mine ? r2_bits : kNone);
    const uint32_t pos_min = wave_umin(mine && r2_bits == r2_min ? pos : kNone);
    if (lane == uint32_t(leader)) {
      atomicMin(&keys[elected], (static_cast<unsigned long long>(r2_min) << 32) | pos_min);
      atomicAdd(&cnts[elected], n);
    }
    live = live && !mine;
  }
  if (live) {
    atomicMin(&keys[cell], (static_cast<unsigned long long>(r2_bits) << 32) | pos);
    atomicAdd(&cnts[cell], 1u);
  }
}

template <int kKind>
__global__ __launch_bounds__(kThreads) void k_sectors_reduce(const Args a) {
#pragma clang fp contract(off)
  constexpr bool kElevation = kKind == D2PC_SECTORS_LAYERS_ELEVATION;
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(lds);
  uint32_t *cnts = reinterpret_cast<uint32_t *>(keys + a.n_cells);
  float2 *tab = reinterpret_cast<float2 *>(cnts + a.n_cells);   // (n_cells is even: 8-byte aligned)
  [[maybe_unused]] const float2 *etab = tab + a.half;           // n_layers + 1 x (ce, se), behind the azimuth table
  const uint32_t tid = threadIdx.x;
  for (int i = int(tid); i < a.n_cells; i += kThreads) keys[i] = ~0ull, cnts[i] = 0u;
  // (the session's device table holds the elevation table behind the azimuth table, as the LDS does)
  for (int j = int(tid); j < a.half + (kElevation ? a.n_layers + 1 : 0); j += kThreads) tab[j] = a.table[j];
  __syncthreads();

  for (uint64_t share = blockIdx.x; share < a.shares; share += uint64_t(a.blocks)) {
    uint64_t cloud = 0;
    uint32_t in_cloud = uint32_t(share);
    if (a.n_clouds > 1) {
      cloud = share / a.shares_per_cloud;
      in_cloud = uint32_t(share - cloud * a.shares_per_cloud);
    }
    uint32_t n = a.cloud_points;
    if (a.counts) {
      const uint32_t given = a.counts[cloud];
      n = given == 0xFFFFFFFFu ? 0u : min(given, a.cloud_points);
    }
    const uint32_t i0 = in_cloud * uint32_t(D2PC_SECTORS_SHARE_POINTS);   // (< 2^32: shares_per_cloud <= 2^22)
    if (i0 >= n) continue;
    const uint64_t first = cloud * a.stride;   // the cloud's first record in `points`; its position fits 32 bits
    uint4 rec[kPerLane];
    bool have[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const uint32_t i = i0 + uint32_t(k * kThreads) + tid;   // (i0 + 1,023 <= 2^32 - 1: no wrap)
      have[k] = i < n;
      rec[k] = make_uint4(0u, 0u, 0u, 0u);
      if (have[k]) rec[k] = a.points[(first + i) * a.step16];
      asm volatile("" ::"v"(rec[k].w));   // keeps the load a whole 16-byte one (w is not used: it would shrink to 12)
    }
    float f[kPerLane], l[kPerLane];
    uint32_t cell[kPerLane], r2_bits[kPerLane], sector[kPerLane];
    [[maybe_unused]] float up[kPerLane], hz[kPerLane];   // elevation: u and the horizontal range h = sqrtf(r2)
    const float2 t0 = tab[0];
    [[maybe_unused]] float2 lo, hi;   // elevation: the band's two boundaries
    if constexpr (kElevation) lo = etab[0], hi = etab[a.n_layers];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const uint4 p = rec[k];
      const bool finite = (p.x & 0x7F800000u) != 0x7F800000u && (p.y & 0x7F800000u) != 0x7F800000u && (p.z & 0x7F800000u) != 0x7F800000u;
      const float ff = pick(p, a.axis[0], a.flip[0]), ll = pick(p, a.axis[1], a.flip[1]);
      const float u = pick(p, a.axis[2], a.flip[2]);
      const float r2 = ff * ff + ll * ll;
      bool in;
      uint32_t layer = 0;
      float key = r2;
      if constexpr (kElevation) {
        // the band's two boundaries are gates; `!(t >= 0)` and `t >= 0` as written: a NaN t (0 * inf) takes no part
        const float h = __builtin_sqrtf(r2);   // (the correctly rounded one: the file's flags)
        key = r2 + u * u;
        const float t_lo = lo.x * u - lo.y * h, t_hi = hi.x * u - hi.y * h;
        in = have[k] && finite && r2 > 0.0f && key >= a.rmin2 && key <= a.rmax2 && t_lo >= 0.0f && !(t_hi >= 0.0f);
        up[k] = u, hz[k] = h;
      } else {
        in = have[k] && finite && r2 > 0.0f && r2 >= a.rmin2 && r2 <= a.rmax2 && u >= a.u_min && u < a.u_max;
        if (a.n_layers > 1) {
          const float slab = floorf((u - a.u_min) * a.inv_h);
          layer = slab >= float(a.n_layers - 1) ? uint32_t(a.n_layers - 1) : uint32_t(int(slab));   // (in: slab >= 0)
        }
      }
      const float cross0 = t0.x * ll - t0.y * ff, dot0 = t0.x * ff + t0.y * ll;
      // the half turn as a sign-bit mask, without a branch: hipcc of ROCm 7 structurised `if (A || (B && C)) negate` so
      // that the lanes of B && C kept f and l un-negated (tests/test_sectors_gpu.py: l = +-0 with f < 0)
      const uint32_t turn = (uint32_t(cross0 < 0.0f) | (uint32_t(cross0 == 0.0f) & uint32_t(dot0 < 0.0f))) << 31;
      f[k] = __uint_as_float(__float_as_uint(ff) ^ turn), l[k] = __uint_as_float(__float_as_uint(ll) ^ turn);
      sector[k] = turn ? uint32_t(a.half) : 0u;
      cell[k] = in ? layer * uint32_t(a.n_sectors) : kNone;
      r2_bits[k] = __float_as_uint(key);
    }
    // the count of the boundaries behind the point: one LDS read of (c_j, s_j) serves the lane's four records, and
    // every lane reads the same address (a broadcast: no bank conflict)
    for (int j = 1; j < a.half; ++j) {
      const float2 t = tab[j];
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) sector[k] += (t.x * l[k] - t.y * f[k]) >= 0.0f ? 1u : 0u;
    }
    if constexpr (kElevation) {
      // the layer: the interior boundaries at or below the point, counted like the sectors (a compare folded into an add)
      uint32_t layer[kPerLane] = {};
      for (int i = 1; i < a.n_layers; ++i) {
        const float2 t = etab[i];
#pragma unroll
        for (int k = 0; k < kPerLane; ++k) layer[k] += (t.x * up[k] - t.y * hz[k]) >= 0.0f ? 1u : 0u;
      }
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) sector[k] += layer[k] * uint32_t(a.n_sectors);   // (cell[k] is 0 or kNone here)
    }
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const uint32_t c = cell[k] == kNone ? kNone : cell[k] + sector[k];
      merge(keys, cnts, a.rounds, c, r2_bits[k], uint32_t(first) + i0 + uint32_t(k * kThreads) + tid);
    }
  }

  __syncthreads();
  unsigned long long *slab_k = reinterpret_cast<unsigned long long *>(a.slab_keys) + size_t(blockIdx.x) * size_t(a.n_cells);
  uint32_t *slab_c = a.slab_counts + size_t(blockIdx.x) * size_t(a.n_cells);
  for (int i = int(tid); i < a.n_cells; i += kThreads) slab_k[i] = keys[i], slab_c[i] = cnts[i];
}

__global__ __launch_bounds__(kThreads) void k_sectors_finish(const Args a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long sk[kThreads];
  __shared__ uint32_t sc[kThreads];
  const int tid = int(threadIdx.x), slice = tid / kFinishCells;
  const int cell = int(blockIdx.x) * kFinishCells + tid % kFinishCells;
  unsigned long long key = ~0ull;
  uint32_t cnt = 0;
  if (cell < a.n_cells) {
    const unsigned long long *slab_k = reinterpret_cast<const unsigned long long *>(a.slab_keys);
#pragma unroll 8
    for (int b = slice; b < a.blocks; b += kFinishSlices) {
      const size_t at = size_t(b) * size_t(a.n_cells) + size_t(cell);
      const unsigned long long k = slab_k[at];
      key = k < key ? k : key;
      cnt += a.slab_counts[at];
    }
  }
  sk[tid] = key, sc[tid] = cnt;
  for (int s = kFinishSlices / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (slice < s) {
      const unsigned long long k = sk[tid + s * kFinishCells];
      key = k < key ? k : key;
      cnt += sc[tid + s * kFinishCells];
      sk[tid] = key, sc[tid] = cnt;
    }
  }
  if (slice != 0 || cell >= a.n_cells) return;
  const bool seen = cnt >= a.min_count;   // (min_count >= 1: an empty cell is never seen)
  const float range = seen ? __builtin_sqrtf(__uint_as_float(uint32_t(key >> 32))) : __uint_as_float(0x7F800000u);
  if (a.range) a.range[cell] = range;
  if (a.count) a.count[cell] = cnt;
  if (a.nearest) a.nearest[cell] = uint32_t(key);   // (the empty key's low word is the empty mark)
  if (a.distance_cm) {
    const float cm = range * 100.0f;
    a.distance_cm[cell] = uint16_t(!seen ? a.no_obstacle_cm : cm >= 65534.0f ? 65534u : uint32_t(cm));
  }
}

}  // namespace

// the instantiation a session of plan `p` launches
const void *reduce_kernel(const Plan &p) {
  return p.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION ? reinterpret_cast<const void *>(&k_sectors_reduce<D2PC_SECTORS_LAYERS_ELEVATION>)
                                                       : reinterpret_cast<const void *>(&k_sectors_reduce<D2PC_SECTORS_LAYERS_HEIGHT>);
}

int prepare_sectors_kernels(const Plan &p) {
  // beyond 64 KB of dynamic LDS the runtime wants to be told (360 x 16 cells need 70,560 bytes, 90 x 64 elevation cells
  // 70,000), for the instantiation that is launched
  if (p.lds_bytes <= 64u * 1024u) return int(hipSuccess);
  return int(hipFuncSetAttribute(reduce_kernel(p), hipFuncAttributeMaxDynamicSharedMemorySize, int(p.lds_bytes)));
}

int launch_sectors(const Launch &in) {
  Args a;
  a.points = static_cast<const uint4 *>(in.points), a.counts = in.counts;
  a.table = reinterpret_cast<const float2 *>(in.table);
  a.slab_keys = in.slab_keys, a.slab_counts = in.slab_counts;
  a.range = in.range, a.count = in.count, a.nearest = in.nearest, a.distance_cm = in.distance_cm;
  a.stride = in.stride, a.shares = in.shares;
  a.shares_per_cloud = in.shares_per_cloud, a.cloud_points = in.cloud_points, a.n_clouds = in.n_clouds, a.step16 = in.step16;
  const Plan &p = in.plan;
  a.n_sectors = p.n_sectors, a.n_layers = p.n_layers, a.n_cells = p.n_cells, a.half = p.half, a.blocks = in.blocks;
#ifdef D2PC_SECTORS_FORCE_ROUNDS
  a.rounds = D2PC_SECTORS_FORCE_ROUNDS;
#else
  a.rounds = p.n_cells <= kWaveRoundsMaxCells ? kWaveRounds : 0;
#endif
  a.rmin2 = p.rmin2, a.rmax2 = p.rmax2, a.u_min = p.u_min, a.u_max = p.u_max, a.inv_h = p.inv_h;
  for (int i = 0; i < 3; ++i) a.axis[i] = p.axis[i], a.flip[i] = p.flip[i];
  a.min_count = p.min_count, a.no_obstacle_cm = p.no_obstacle_cm;
  hipStream_t s = static_cast<hipStream_t>(in.stream);
  if (p.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION)
    hipLaunchKernelGGL(k_sectors_reduce<D2PC_SECTORS_LAYERS_ELEVATION>, dim3(unsigned(in.blocks)), dim3(kThreads), p.lds_bytes, s, a);
  else
    hipLaunchKernelGGL(k_sectors_reduce<D2PC_SECTORS_LAYERS_HEIGHT>, dim3(unsigned(in.blocks)), dim3(kThreads), p.lds_bytes, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return int(e);
  hipLaunchKernelGGL(k_sectors_finish, dim3(unsigned((p.n_cells + kFinishCells - 1) / kFinishCells)), dim3(kThreads), 0, s, a);
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
