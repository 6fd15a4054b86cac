// d2pc_sectors_relief.hip -- the kernels of the relief session of include/d2pc_sectors.h (gfx950).
//
// k_relief_window    MANY blocks of 256 lanes, k_slope_merge's shape: 16 cells x 16 slices, cell = lane % 16, so consecutive
//                    lanes read consecutive cells of a plane.  Every block loads the 16 headers to LDS and computes the
//                    anchor, the slot choice and the list of the slots that take part identically
//                    (d2pc_sectors_terrain_ring.hpp: the terrain's own code).  Slice 0 is the frame, slice s the (s - 1)-th
//                    entry of the list: a lane issues the ten loads of its cell's entry -- nine 64-bit planes and the count,
//                    at the shifted index for a stored table -- before anything is added; the lane of slice 0 stores the
//                    frame's entry to slot v with plain vector stores.  Then k_slope_merge's tree through LDS over the
//                    slices, and one lane a cell runs the fit (d2pc_sectors_slope_fit.hpp: the slope's own code), writes the
//                    per-cell outputs the caller asked for and the 14 bytes per cell that the sites read.  No block writes a
//                    header and no block reads slot v (v is never in the list): there is no order to keep between blocks.
// k_relief_sites     ONE block of 1,024 lanes.  It derives the slot choice again from the old headers; behind the barrier
//                    that follows every header read lane 0 commits the new header (the restart's zeroed headers come from
//                    the lanes beside it) and writes status; then, when site, candidates or summary is asked for, the
//                    slope's site stage from the hand-on buffer.  A frame that is not anchored commits nothing.
// k_relief_reset     16 lanes, one 16-byte vector store each: the headers are zero again.
// No global atomic, nothing to clear.  Every accumulated value is an integer and wraps as the specification says; the two
// float products of the anchor and every double operation of the fit are rounded once: contraction is off in this file.
#include <hip/hip_runtime.h>

#include "d2pc_sectors_relief_plan.hpp"
#include "d2pc_sectors_slope_fit.hpp"
#include "d2pc_sectors_terrain_ring.hpp"

namespace d2pc {
namespace sectors {
namespace {

struct ReliefArgs {   // ReliefLaunch without its host-only members
  uint4 *headers;                // the state block: 16 headers ...
  unsigned char *tables;         // ... and, 256 bytes on, `depth` tables of slot_bytes
  size_t slot_bytes;
  uint32_t *hand_on;
  const uint32_t *step;          // the 20 words of a d2pc_sectors_ground_step
  const uint32_t *frame_count;
  const unsigned long long *frame_sum, *frame_sum2, *frame_moments;
  const uint8_t *allowed;
  uint32_t *count;
  unsigned long long *sum, *sum2, *moments;
  uint32_t *slope_a, *slope_b, *level_q, *resid_q2;
  uint8_t *flat, *site;
  unsigned long long *candidates;
  uint32_t *summary, *status;
  int depth, n_candidates;
  GroundSiteGrid grid;
  float inv_c;
  SlopeFit fit;
};

__device__ __forceinline__ unsigned long long *table_of(const ReliefArgs &a, int slot) {
  return reinterpret_cast<unsigned long long *>(a.tables + size_t(slot) * a.slot_bytes);
}

// what every block of both launches derives from the same 16 headers: they go to LDS, and behind the barrier the anchor, the
// slot choice and (from wave 0) the list are the same in every lane.  All lanes of the block call it.
struct ReliefRing {
  uint4 hdr[D2PC_SECTORS_TERRAIN_MAX_DEPTH];
  int part_slot[D2PC_SECTORS_TERRAIN_MAX_DEPTH], part_di[D2PC_SECTORS_TERRAIN_MAX_DEPTH], part_dj[D2PC_SECTORS_TERRAIN_MAX_DEPTH];
  int part_n;
};

__device__ __forceinline__ void relief_ring(const ReliefArgs &a, ReliefRing &ring, TerrainAnchor *an, TerrainSlot *sl) {
  const int tid = int(threadIdx.x);
  if (tid < a.depth) ring.hdr[tid] = a.headers[tid];
  *an = terrain_anchor(a.step, a.inv_c);
  __syncthreads();   // every read of a header in device memory lies before this barrier
  *sl = terrain_slot_choice(ring.hdr, a.depth);
  if (tid < 64)
    terrain_participants(ring.hdr, a.depth, a.grid.n_a, a.grid.n_b, *an, *sl, tid, ring.part_slot, ring.part_di, ring.part_dj, &ring.part_n);
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void k_relief_window(const ReliefArgs a) {
  __shared__ ReliefRing ring;
  __shared__ unsigned long long sw[kSlopeWords][kThreads];
  __shared__ uint32_t sc[kThreads];
  TerrainAnchor an;
  TerrainSlot sl;
  relief_ring(a, ring, &an, &sl);
  const int tid = int(threadIdx.x), slice = tid / kReliefCells;
  const int cell = int(blockIdx.x) * kReliefCells + tid % kReliefCells;
  const int n_cells = a.grid.n_cells, n_a = a.grid.n_a, n_b = a.grid.n_b;
  const int n_part = ring.part_n;

  // ---- the lane's entry: the frame's (entry 0) or a listed table's at the shifted index; its ten loads are issued before
  // anything is added (entry e = slice + t x slices: one entry a lane in the 16 x 16 shape)
  unsigned long long s[kSlopeWords] = {};
  uint32_t cnt = 0;
  if (cell < n_cells && an.anchored) {
#pragma unroll
    for (int t = 0; t < kReliefPerLane; ++t) {
      const int e = slice + t * kReliefSlices;
      if (e == 0) {
        s[0] = a.frame_sum[cell], s[1] = a.frame_sum2[cell];
#pragma unroll
        for (int p = 0; p < D2PC_SECTORS_SLOPE_MOMENTS; ++p) s[2 + p] = a.frame_moments[size_t(p) * size_t(n_cells) + cell];
        cnt = a.frame_count[cell];
        unsigned long long *own = table_of(a, sl.v);   // (no lane of any block reads slot v)
#pragma unroll
        for (int p = 0; p < kSlopeWords; ++p) own[size_t(p) * size_t(n_cells) + cell] = s[p];
        reinterpret_cast<uint32_t *>(own + size_t(kSlopeWords) * size_t(n_cells))[cell] = cnt;
      } else if (e - 1 < n_part) {
        const int j = cell / n_a, i = cell - j * n_a;
        const int ii = i + ring.part_di[e - 1], jj = j + ring.part_dj[e - 1];
        if (ii >= 0 && ii < n_a && jj >= 0 && jj < n_b) {
          const int o = jj * n_a + ii;   // 0 .. n_cells - 1
          const unsigned long long *tb = table_of(a, ring.part_slot[e - 1]);
          unsigned long long v[kSlopeWords];
#pragma unroll
          for (int p = 0; p < kSlopeWords; ++p) v[p] = tb[size_t(p) * size_t(n_cells) + o];
          const uint32_t vc = reinterpret_cast<const uint32_t *>(tb + size_t(kSlopeWords) * size_t(n_cells))[o];
#pragma unroll
          for (int p = 0; p < kSlopeWords; ++p) s[p] += v[p];
          cnt += vc;
        }
      }
    }
  }

  // ---- k_slope_merge's tree over the slices
#pragma unroll
  for (int p = 0; p < kSlopeWords; ++p) sw[p][tid] = s[p];
  sc[tid] = cnt;
  for (int h = kReliefSlices / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (slice < h) {
#pragma unroll
      for (int p = 0; p < kSlopeWords; ++p) s[p] += sw[p][tid + h * kReliefCells], sw[p][tid] = s[p];
      cnt += sc[tid + h * kReliefCells], sc[tid] = cnt;
    }
  }
  if (slice != 0 || cell >= n_cells) return;

  // ---- 5. the slope's fit and per-cell outputs, of the window
  const SlopeCell o = slope_cell_fit(a.fit, cnt, s);
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

__global__ __launch_bounds__(kGroundSiteThreads) void k_relief_sites(const ReliefArgs a) {
  __shared__ GroundSiteLds lds;
  __shared__ uint32_t fit_slot[kGroundSiteWaves];
  __shared__ ReliefRing ring;
  TerrainAnchor an;
  TerrainSlot sl;
  relief_ring(a, ring, &an, &sl);   // from the OLD headers: the window launch wrote none
  const int tid = int(threadIdx.x);
  if (an.anchored) {   // (uniform)
    if (tid == 0) a.headers[sl.v] = make_uint4(uint32_t(an.ia0), uint32_t(an.jb0), an.h0_bits, sl.q);
    else if (sl.restart && tid < a.depth) a.headers[tid] = make_uint4(0u, 0u, 0u, 0u);   // (v is 0 then)
  }
  if (tid == 0 && a.status) {
    a.status[0] = an.anchored ? sl.q : sl.largest, a.status[1] = an.anchored ? uint32_t(ring.part_n) + 1u : 0u;
    a.status[2] = uint32_t(an.ia0), a.status[3] = uint32_t(an.jb0);   // (both 0 when not anchored)
  }
  if (!(a.site || a.candidates || a.summary)) return;   // (uniform: kernel arguments)
  GroundSiteStage st;
  st.grid = a.grid, st.n_candidates = a.n_candidates;
  st.goal_i = a.step[15], st.goal_j = a.step[16];
  st.allowed = a.allowed, st.site = a.site, st.candidates = a.candidates, st.summary = a.summary;
  slope_sites_from_hand_on(a.hand_on, st, lds, fit_slot);
}

__global__ __launch_bounds__(64) void k_relief_reset(uint4 *headers) {
  if (threadIdx.x < D2PC_SECTORS_TERRAIN_MAX_DEPTH) headers[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

int launch_relief(const ReliefLaunch &in) {
  const d2pc_sectors_relief_desc &d = *in.desc;
  ReliefArgs a;
  a.headers = static_cast<uint4 *>(in.state);
  a.tables = static_cast<unsigned char *>(in.state) + kTerrainHeadersBytes;
  a.slot_bytes = in.plan.slot_bytes;
  a.hand_on = static_cast<uint32_t *>(in.hand_on);
  a.step = reinterpret_cast<const uint32_t *>(d.step), a.frame_count = d.frame_count;
  a.frame_sum = reinterpret_cast<const unsigned long long *>(d.frame_sum), a.frame_sum2 = reinterpret_cast<const unsigned long long *>(d.frame_sum2);
  a.frame_moments = reinterpret_cast<const unsigned long long *>(d.frame_moments);
  a.allowed = d.allowed;
  a.count = d.count, a.sum = reinterpret_cast<unsigned long long *>(d.sum), a.sum2 = reinterpret_cast<unsigned long long *>(d.sum2);
  a.moments = reinterpret_cast<unsigned long long *>(d.moments);
  a.slope_a = reinterpret_cast<uint32_t *>(d.slope_a), a.slope_b = reinterpret_cast<uint32_t *>(d.slope_b);
  a.level_q = reinterpret_cast<uint32_t *>(d.level_q), a.resid_q2 = d.resid_q2, a.flat = d.flat, a.site = d.site;
  a.candidates = reinterpret_cast<unsigned long long *>(d.candidates), a.summary = d.summary, a.status = d.status;
  a.depth = in.plan.depth, a.n_candidates = d.candidates ? d.n_candidates : 0;
  const GroundPlan &g = in.plan.slope.ground;
  a.grid = ground_site_grid(g), a.inv_c = g.inv_c;
  a.fit = slope_fit_of(in.plan.slope);
  hipStream_t s = static_cast<hipStream_t>(in.stream);
  hipLaunchKernelGGL(k_relief_window, dim3(unsigned(in.plan.blocks)), dim3(kThreads), 0, s, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return int(e);
  hipLaunchKernelGGL(k_relief_sites, dim3(1), dim3(kGroundSiteThreads), 0, s, a);   // (always: the header is committed here)
  return int(hipGetLastError());
}

int launch_relief_reset(void *state, void *stream) {
  hipLaunchKernelGGL(k_relief_reset, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<uint4 *>(state));
  return int(hipGetLastError());
}

}  // namespace sectors
}  // namespace d2pc
