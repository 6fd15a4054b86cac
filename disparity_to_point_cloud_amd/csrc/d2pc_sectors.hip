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
//                    Where a record falls (picks, gates, half turn, a step of either boundary count, the key's bits) is
//                    d2pc_sectors_bin.hpp's, which the memory's kernel calls too; the walk over the shares and its loads, and
//                    the wave minimum, are d2pc_sectors_device.hpp's; here are the two loops' skeletons and the tables of cells.
// k_sectors_finish   min / sum over the slabs, coalesced across cells (8 cells x 32 slices of the slabs per block, a
//                    tree through LDS over the slices), then the outputs the caller asked for.
// Keys are integers and counts are sums of integers: the result is the same bytes whatever order lanes, waves and
// blocks arrive in.  Every float expression of the specification is rounded once: contraction is off in this file.
#include <hip/hip_runtime.h>

#include "d2pc_sectors_bin.hpp"

namespace d2pc {
namespace sectors {
namespace {

[[maybe_unused]] constexpr int kWaveRounds = 2;   // elected cells per wave and record slot ...
[[maybe_unused]] constexpr int kWaveRoundsMaxCells = 72;   // ... for grids up to this many cells; none beyond
constexpr int kFinishCells = 8, kFinishSlices = 32;
static_assert(kFinishCells * kFinishSlices == kThreads, "the finishing block is cells x slices");

// Launch without its host-only members.  The walk's eight fields stand here one by one, where they stood before CloudWalk:
// embedded as the struct (at the front, behind the outputs or at the end alike) hipcc of ROCm 7 allocates k_sectors_reduce
// 64 / 52 VGPRs for 68 / 68 and schedules it anew, and S came out 2 to 7 % slower in all four rows
// (profiles/sectors_shared_bench.txt).  With the fields here and the struct made of them in the kernel, the shared walk
// compiles to the instruction stream it had.  GroundArgs embeds the struct: k_ground_reduce is the same either way.
struct Args {
  const void *points;
  const uint32_t *counts;
  const float2 *table;
  uint64_t *slab_keys;
  uint32_t *slab_counts;
  float *range;
  uint32_t *count, *nearest;
  uint16_t *distance_cm;
  uint64_t stride, shares;
  uint32_t shares_per_cloud, cloud_points, n_clouds, step16;
  int blocks, rounds;
  GridArgs grid;
};

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
  const GridArgs g = a.grid;
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(lds);
  uint32_t *cnts = reinterpret_cast<uint32_t *>(keys + g.n_cells);
  float2 *tab = reinterpret_cast<float2 *>(cnts + g.n_cells);   // (n_cells is even: 8-byte aligned)
  const uint32_t tid = threadIdx.x;
  for (int i = int(tid); i < g.n_cells; i += kThreads) keys[i] = ~0ull, cnts[i] = 0u;
  // (the session's device table holds the elevation table, n_layers + 1 x (ce, se), behind the azimuth table, as the LDS does)
  for (int j = int(tid); j < g.half + (kElevation ? g.n_layers + 1 : 0); j += kThreads) tab[j] = a.table[j];
  __syncthreads();

  const CloudWalk walk = {a.points, a.counts, a.stride, a.shares, a.shares_per_cloud, a.cloud_points, a.n_clouds, a.step16};
  for (uint64_t share = blockIdx.x; share < walk.shares; share += uint64_t(a.blocks)) {
    ShareAt at;
    if (!find_share(walk, share, &at)) continue;   // (d2pc_sectors_device.hpp)
    uint4 rec[kPerLane];
    bool have[kPerLane];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) rec[k] = share_record(walk, at, tid, k, &have[k]);
    // where the lane's four records fall (d2pc_sectors_bin.hpp)
    float f[kPerLane], l[kPerLane], up[kPerLane], hz[kPerLane];
    uint32_t cell[kPerLane], key_bits[kPerLane], sector[kPerLane], layer[kPerLane] = {};
    const float2 t0 = tab[0], lo = tab[kElevation ? g.half : 0], hi = tab[kElevation ? g.half + g.n_layers : 0];
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      const Binned b = bin_record<kElevation, const uint4 &>(g, t0, lo, hi, rec[k], have[k]);
      f[k] = b.f, l[k] = b.l, up[k] = b.up, hz[k] = b.hz, cell[k] = b.cell, key_bits[k] = b.key_bits, sector[k] = b.sector;
    }
    for (int j = 1; j < g.half; ++j) {
      const float2 t = tab[j];
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) sector[k] += behind(t, l[k], f[k]);
    }
    for (int i = 1; kElevation && i < g.n_layers; ++i) {
      const float2 t = tab[g.half + i];
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) layer[k] += behind(t, up[k], hz[k]);
    }
#pragma unroll
    for (int k = 0; k < kPerLane; ++k)
      merge(keys, cnts, a.rounds, cell_of(g, cell[k], sector[k], layer[k]), key_bits[k], share_position(at, tid, k));
  }

  __syncthreads();
  unsigned long long *slab_k = reinterpret_cast<unsigned long long *>(a.slab_keys) + size_t(blockIdx.x) * size_t(g.n_cells);
  uint32_t *slab_c = a.slab_counts + size_t(blockIdx.x) * size_t(g.n_cells);
  for (int i = int(tid); i < g.n_cells; i += kThreads) slab_k[i] = keys[i], slab_c[i] = cnts[i];
}

__global__ __launch_bounds__(kThreads) void k_sectors_finish(const Args a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long sk[kThreads];
  __shared__ uint32_t sc[kThreads];
  const int tid = int(threadIdx.x), slice = tid / kFinishCells;
  const int cell = int(blockIdx.x) * kFinishCells + tid % kFinishCells;
  const int n_cells = a.grid.n_cells;
  unsigned long long key = ~0ull;
  uint32_t cnt = 0;
  if (cell < n_cells) {
    const unsigned long long *slab_k = reinterpret_cast<const unsigned long long *>(a.slab_keys);
#pragma unroll 8
    for (int b = slice; b < a.blocks; b += kFinishSlices) {
      const size_t at = size_t(b) * size_t(n_cells) + size_t(cell);
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
  if (slice != 0 || cell >= n_cells) return;
  const bool seen = cnt >= a.grid.min_count;   // (min_count >= 1: an empty cell is never seen)
  const float range = seen ? range_of_key(key) : __uint_as_float(0x7F800000u);
  if (a.range) a.range[cell] = range;
  if (a.count) a.count[cell] = cnt;
  if (a.nearest) a.nearest[cell] = uint32_t(key);   // (the empty key's low word is the empty mark)
  if (a.distance_cm) a.distance_cm[cell] = distance_cm_of(a.grid, range, !seen);
}

// the instantiation a session of plan `p` launches: the one place that turns a layer kind into a kernel
const void *reduce_kernel(const Plan &p) {
  return p.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION ? reinterpret_cast<const void *>(&k_sectors_reduce<D2PC_SECTORS_LAYERS_ELEVATION>)
                                                       : reinterpret_cast<const void *>(&k_sectors_reduce<D2PC_SECTORS_LAYERS_HEIGHT>);
}

}  // namespace

int prepare_sectors_kernels(const Plan &p) {
  // beyond 64 KB of dynamic LDS the runtime wants to be told (360 x 16 cells need 70,560 bytes, 90 x 64 elevation cells
  // 70,000), for the instantiation that is launched
  if (p.lds_bytes <= 64u * 1024u) return int(hipSuccess);
  return int(hipFuncSetAttribute(reduce_kernel(p), hipFuncAttributeMaxDynamicSharedMemorySize, int(p.lds_bytes)));
}

int launch_sectors(const Launch &in) {
  Args a;
  const CloudWalk &w = in.walk;
  a.points = w.points, a.counts = w.counts, a.stride = w.stride, a.shares = w.shares;
  a.shares_per_cloud = w.shares_per_cloud, a.cloud_points = w.cloud_points, a.n_clouds = w.n_clouds, a.step16 = w.step16;
  a.table = reinterpret_cast<const float2 *>(in.table);
  a.slab_keys = in.slab_keys, a.slab_counts = in.slab_counts;
  a.range = in.range, a.count = in.count, a.nearest = in.nearest, a.distance_cm = in.distance_cm;
  const Plan &p = in.plan;
  a.grid = grid_args(p), a.blocks = in.blocks;
#ifdef D2PC_SECTORS_FORCE_ROUNDS
  a.rounds = D2PC_SECTORS_FORCE_ROUNDS;
#else
  a.rounds = p.n_cells <= kWaveRoundsMaxCells ? kWaveRounds : 0;
#endif
  hipStream_t s = static_cast<hipStream_t>(in.stream);
  void *args[] = {&a};
  (void)hipLaunchKernel(reduce_kernel(p), dim3(unsigned(in.blocks)), dim3(kThreads), args, p.lds_bytes, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return int(e);
  hipLaunchKernelGGL(k_sectors_finish, dim3(unsigned((p.n_cells + kFinishCells - 1) / kFinishCells)), dim3(kThreads), 0, s, a);
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
