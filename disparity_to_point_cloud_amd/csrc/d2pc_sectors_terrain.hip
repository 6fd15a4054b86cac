// d2pc_sectors_terrain.hip -- the kernels of the terrain session of include/d2pc_sectors.h (gfx950).
//
// k_terrain_update   ONE block of 1,024 lanes, four cells a lane at the most, lane <-> cell as k_ground_sites has it (cell
//                    tid + k x 1,024): consecutive lanes read consecutive cells of a stored table's shifted row.
//                    The 16-byte headers of the `depth` slots go to LDS first; behind the barrier every lane computes the
//                    slot choice (the smallest seq is replaced, the largest + 1 is the new one) identically from them, and
//                    wave 0 compacts the slots that take part (seq != 0, the same h0, a shift that leaves some of the grid
//                    in sight) into a list in LDS by one ballot -- a slot whose shift leaves the grid is never in the list,
//                    so no lane visits it.  Per cell the loads of a batch of kTerrainBatch listed tables are issued before
//                    the first add: 8 + 8 + 4 bytes each, unconditional (a cell the shift carries out of the grid reads
//                    its own index and adds zero), so they are in flight together.  The lane that reads the frame's entry
//                    stores it to slot v: plain vector stores, and no lane reads slot v, so there is no order to keep.
//                    The new header is written by lane 0 behind the barrier that follows every header read.  mean_q and
//                    flat go to LDS and spread_q2 stays in registers: the kernel runs straight into the ground's site
//                    stage (d2pc_sectors_ground_sites.hpp).  No global atomic, nothing to clear.
// k_terrain_reset    16 lanes, one 16-byte vector store each: the headers are zero again.
// Every accumulated value is an integer and wraps as the specification says.  The two float products of the anchor are
// rounded once: contraction is off in this file.
#include <hip/hip_runtime.h>

#include "d2pc_sectors_ground_sites.hpp"
#include "d2pc_sectors_terrain_ring.hpp"

namespace d2pc {
namespace sectors {
namespace {

// stored tables whose loads are in flight together per cell: the default depth's 7 in one batch, depth 16's 15 in two.  16 wide
// alone compiles to 105 VGPRs and issues 9 idle loads a cell at the default depth; 8 and 16 wide side by side behind a uniform
// branch spill (128 VGPRs and 140 bytes of scratch a lane)
constexpr int kTerrainBatch = 8;

struct TerrainArgs {   // TerrainLaunch without its host-only members
  uint4 *headers;                // the state block: 16 headers ...
  unsigned char *tables;         // ... and, 256 bytes on, `depth` tables of slot_bytes
  size_t slot_bytes;
  const uint32_t *step;          // the 20 words of a d2pc_sectors_ground_step
  const uint32_t *frame_count;
  const unsigned long long *frame_sum, *frame_sum2;
  const uint8_t *allowed;
  uint32_t *count;
  unsigned long long *sum, *sum2;
  uint32_t *mean_q, *spread_q2;
  uint8_t *flat, *site;
  unsigned long long *candidates;
  uint32_t *summary, *status;
  int depth, n_candidates;
  GroundSiteGrid grid;
  float inv_c;
  uint32_t min_count, max_spread_q2;
};

__device__ __forceinline__ unsigned long long *table_of(const TerrainArgs &a, int slot) {
  return reinterpret_cast<unsigned long long *>(a.tables + size_t(slot) * a.slot_bytes);
}

// The entries of cell c = (i, j) in the n_part listed tables, added to cnt / sum / sum2, in batches of kTerrainBatch tables.
// The loads of a batch are issued before its first add: 8 + 8 + 4 bytes each and unconditional -- a list entry past n_part
// reads the batch's first entry again and a cell that the shift carries out of the grid reads its own index, and both add
// zero -- so they are in flight together.
__device__ __forceinline__ void add_stored(const TerrainArgs &a, const int *part_slot, const int *part_di, const int *part_dj, int n_part, int c,
                                           int i, int j, uint32_t &cnt, unsigned long long &sum, unsigned long long &sum2) {
  const int n_a = a.grid.n_a, n_b = a.grid.n_b, n_cells = a.grid.n_cells;
  for (int p0 = 0; p0 < n_part; p0 += kTerrainBatch) {
    unsigned long long s1[kTerrainBatch], s2[kTerrainBatch];
    uint32_t sc[kTerrainBatch];
    bool in[kTerrainBatch];
#pragma unroll
    for (int u = 0; u < kTerrainBatch; ++u) {
      const bool listed = p0 + u < n_part;            // (uniform)
      const int p = listed ? p0 + u : p0;
      const int ii = i + part_di[p], jj = j + part_dj[p];
      in[u] = listed && ii >= 0 && ii < n_a && jj >= 0 && jj < n_b;
      const int o = in[u] ? jj * n_a + ii : c;        // 0 .. n_cells - 1 either way
      const unsigned long long *t = table_of(a, part_slot[p]);
      s1[u] = t[o], s2[u] = t[n_cells + o];
      sc[u] = reinterpret_cast<const uint32_t *>(t + 2 * size_t(n_cells))[o];
    }
#pragma unroll
    for (int u = 0; u < kTerrainBatch; ++u) {
      sum += in[u] ? s1[u] : 0ull, sum2 += in[u] ? s2[u] : 0ull;
      cnt += in[u] ? sc[u] : 0u;
    }
  }
}

__global__ __launch_bounds__(kGroundSiteThreads) void k_terrain_update(const TerrainArgs a) {
#pragma clang fp contract(off)
  __shared__ GroundSiteLds lds;
  __shared__ uint4 hdr[D2PC_SECTORS_TERRAIN_MAX_DEPTH];
  __shared__ int part_slot[D2PC_SECTORS_TERRAIN_MAX_DEPTH], part_di[D2PC_SECTORS_TERRAIN_MAX_DEPTH], part_dj[D2PC_SECTORS_TERRAIN_MAX_DEPTH];
  __shared__ int part_n;
  const int tid = int(threadIdx.x);
  const int n_cells = a.grid.n_cells, n_a = a.grid.n_a, n_b = a.grid.n_b, depth = a.depth;
  if (tid < depth) hdr[tid] = a.headers[tid];
  // ---- 1. the anchor: the same words in every lane (steps 1, 3 and 4 are d2pc_sectors_terrain_ring.hpp's)
  const TerrainAnchor an = terrain_anchor(a.step, a.inv_c);
  const uint32_t h0_bits = an.h0_bits;
  const bool anchored = an.anchored;
  const int ia0 = an.ia0, jb0 = an.jb0;
  __syncthreads();   // every read of a header in device memory lies before this barrier

  // ---- 3. the slot choice, identically in every lane
  const TerrainSlot sl = terrain_slot_choice(hdr, depth);
  const uint32_t largest = sl.largest, q = sl.q;
  const bool restart = sl.restart;
  const int v = sl.v;

  // ---- 4. the slots that take part, compacted by wave 0 (all 64 lanes of it are here: the ballot is whole)
  if (tid < 64) terrain_participants(hdr, depth, n_a, n_b, an, sl, tid, part_slot, part_di, part_dj, &part_n);
  __syncthreads();
  const int n_part = part_n;

  if (anchored) {   // (uniform)
    if (tid == 0) a.headers[v] = make_uint4(uint32_t(ia0), uint32_t(jb0), h0_bits, q);
    else if (restart && tid < depth) a.headers[tid] = make_uint4(0u, 0u, 0u, 0u);   // (v is 0 then)
  }
  if (tid == 0 && a.status) {
    a.status[0] = anchored ? q : largest, a.status[1] = anchored ? uint32_t(n_part) + 1u : 0u;
    a.status[2] = uint32_t(ia0), a.status[3] = uint32_t(jb0);   // (both 0 when not anchored)
  }

  unsigned long long *own = table_of(a, v);
  uint32_t *own_c = reinterpret_cast<uint32_t *>(own + 2 * size_t(n_cells));
  uint32_t points = 0, n_flat = 0;
  uint32_t spread[kGroundPerLane] = {};
#pragma unroll
  for (int k = 0; k < kGroundPerLane; ++k) {
    const int c = tid + k * kGroundSiteThreads;
    if (c >= n_cells) continue;
    uint32_t cnt = 0u;
    unsigned long long sum = 0ull, sum2 = 0ull;
    if (anchored) {
      cnt = a.frame_count[c], sum = a.frame_sum[c], sum2 = a.frame_sum2[c];
      own[c] = sum, own[n_cells + c] = sum2, own_c[c] = cnt;
      if (n_part > 0) {
        const int j = c / n_a, i = c - j * n_a;
        add_stored(a, part_slot, part_di, part_dj, n_part, c, i, j, cnt, sum, sum2);
      }
    }
    // ---- 5. the ground's per-cell outputs, of the window
    uint32_t mean, sp;
    ground_cell_formula(cnt, sum, sum2, &mean, &sp);
    const uint8_t flat = cnt >= a.min_count && sp <= a.max_spread_q2 ? 1 : 0;
    if (a.count) a.count[c] = cnt;
    if (a.sum) a.sum[c] = sum;
    if (a.sum2) a.sum2[c] = sum2;
    if (a.mean_q) a.mean_q[c] = mean;
    if (a.spread_q2) a.spread_q2[c] = sp;
    if (a.flat) a.flat[c] = flat;
    lds.mean_q[c] = int(mean), lds.flat[c] = flat;
    spread[k] = sp, points += cnt, n_flat += flat;
  }
  if (!(a.site || a.candidates || a.summary)) return;   // (uniform: kernel arguments)
  GroundSiteStage st;
  st.grid = a.grid, st.n_candidates = a.n_candidates;
  st.goal_i = a.step[15], st.goal_j = a.step[16];
  st.allowed = a.allowed, st.site = a.site, st.candidates = a.candidates, st.summary = a.summary;
  ground_site_stage(st, lds, spread, points, n_flat);
}

__global__ __launch_bounds__(64) void k_terrain_reset(uint4 *headers) {
  if (threadIdx.x < D2PC_SECTORS_TERRAIN_MAX_DEPTH) headers[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

int launch_terrain(const TerrainLaunch &in) {
  TerrainArgs a;
  a.headers = static_cast<uint4 *>(in.state);
  a.tables = static_cast<unsigned char *>(in.state) + kTerrainHeadersBytes;
  a.slot_bytes = in.plan.slot_bytes;
  a.step = static_cast<const uint32_t *>(in.step), a.frame_count = in.frame_count;
  a.frame_sum = reinterpret_cast<const unsigned long long *>(in.frame_sum), a.frame_sum2 = reinterpret_cast<const unsigned long long *>(in.frame_sum2);
  a.allowed = in.allowed;
  a.count = in.count, a.sum = reinterpret_cast<unsigned long long *>(in.sum), a.sum2 = reinterpret_cast<unsigned long long *>(in.sum2);
  a.mean_q = reinterpret_cast<uint32_t *>(in.mean_q), a.spread_q2 = in.spread_q2, a.flat = in.flat, a.site = in.site;
  a.candidates = static_cast<unsigned long long *>(in.candidates), a.summary = in.summary, a.status = in.status;
  a.depth = in.plan.depth, a.n_candidates = in.candidates ? in.n_candidates : 0;
  const GroundPlan &p = in.plan.ground;
  a.grid = ground_site_grid(p), a.inv_c = p.inv_c;
  a.min_count = p.min_count, a.max_spread_q2 = p.max_spread_q2;
  hipLaunchKernelGGL(k_terrain_update, dim3(1), dim3(kGroundSiteThreads), 0, static_cast<hipStream_t>(in.stream), a);
  return int(hipGetLastError());
}

int launch_terrain_reset(void *state, void *stream) {
  hipLaunchKernelGGL(k_terrain_reset, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<uint4 *>(state));
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
