// d2pc_sectors_relief_plan.hpp -- the host side of the relief session of include/d2pc_sectors.h that needs no device: what
// the three configurations and a relief descriptor are refused for, the sizes of the state block (16 headers, then `depth`
// tables in the slope slab's order), the blocks of the window launch and the overlap of a descriptor with the state.  The
// grid's and the fit's parts are d2pc_sectors_slope_plan.hpp's (make_slope_plan), the depth's d2pc_sectors_terrain_plan.hpp's
// (make_terrain_plan).  Host code only and no device runtime: plain g++ compiles it (tests/test_sectors_relief_cpu.py,
// tests/cpp/sectors_relief_plan_main.cpp).
#pragma once
#include "d2pc_sectors_slope_plan.hpp"
#include "d2pc_sectors_terrain_plan.hpp"

namespace d2pc {
namespace sectors {

// cells of a block of the window launch x slices of the list (the frame and up to 15 stored tables): 16 x 16, k_slope_merge's
// shape, a slice per list entry.  -DD2PC_SECTORS_RELIEF_CELLS=64 (make sectors SNAME=... SDEFS=...) builds the 64 x 4 arm of
// tools/sectors_bench.py --relief, whose lanes take four entries each: DESIGN.md 8j has the measurement
#ifndef D2PC_SECTORS_RELIEF_CELLS
#define D2PC_SECTORS_RELIEF_CELLS 16
#endif
constexpr int kReliefCells = D2PC_SECTORS_RELIEF_CELLS;
constexpr int kReliefSlices = kThreads / kReliefCells;
constexpr int kReliefPerLane = D2PC_SECTORS_TERRAIN_MAX_DEPTH / kReliefSlices;   // list entries a lane takes: 1
static_assert(kReliefCells * kReliefSlices == kThreads && kReliefPerLane * kReliefSlices == D2PC_SECTORS_TERRAIN_MAX_DEPTH,
              "the window block is cells x slices, and the slices cover the frame and depth - 1 slots");
static_assert(D2PC_SECTORS_RELIEF_CELLS != 16 || (kReliefCells == kGroundMergeCells && kReliefSlices == kGroundMergeSlices), "k_slope_merge's shape");

struct ReliefPlan {
  SlopePlan slope;      // the grid (slope.ground) and the fit
  int depth;
  int blocks;           // of the window launch: 16 cells each
  size_t slot_bytes;    // 76 bytes per cell, rounded up to a multiple of 16
  size_t state_bytes;   // the headers and `depth` tables
};

// D2PC_OK and *p filled, or the refusal (and its reason in msg, when given): first d2pc_sectors_slope_geometry's -- the
// ground's, the slope's, the table's size --, then the terrain configuration's, each unchanged
inline int make_relief_plan(const d2pc_sectors_ground_config *g, const d2pc_sectors_slope_config *s, const d2pc_sectors_terrain_config *c,
                            ReliefPlan *p, char *msg = nullptr, size_t msg_len = 0) {
  if (const int st = make_slope_plan(g, s, &p->slope, msg, msg_len)) return st;
  TerrainPlan t;
  if (const int st = make_terrain_plan(g, c, &t, msg, msg_len)) return st;   // (the ground's part has passed: the depth's refusals)
  const size_t n = size_t(p->slope.ground.n_cells);
  p->depth = t.depth;
  p->blocks = int((n + size_t(kReliefCells) - 1u) / size_t(kReliefCells));
  p->slot_bytes = (kSlopeCellBytes * n + 15u) / 16u * 16u;
  p->state_bytes = kTerrainHeadersBytes + size_t(p->depth) * p->slot_bytes;
  return D2PC_OK;
}

inline void fill_relief_geometry(const ReliefPlan &p, d2pc_sectors_relief_geometry_t *g) {
  memset(g, 0, sizeof *g);
  g->n_cells = p.slope.ground.n_cells, g->inv_c = p.slope.ground.inv_c;
  g->slot_bytes = p.slot_bytes, g->state_bytes = p.state_bytes;
  g->headers_offset = 0, g->tables_offset = kTerrainHeadersBytes;
  g->scale = p.slope.scale, g->max_tilt2 = p.slope.max_tilt2;
  g->blocks = p.blocks;
}

constexpr int kReliefInputs = 6, kReliefOutputs = 13;

// the buffers of a descriptor and their sizes: the inputs first
inline void relief_buffers(const ReliefPlan &p, const d2pc_sectors_relief_desc *d, const void *(&bufs)[kReliefInputs + kReliefOutputs],
                           size_t (&bytes)[kReliefInputs + kReliefOutputs]) {
  const size_t n = size_t(p.slope.ground.n_cells);
  const void *b[kReliefInputs + kReliefOutputs] = {d->step, d->frame_count, d->frame_sum, d->frame_sum2, d->frame_moments, d->allowed,
                                                   d->count, d->sum, d->sum2, d->moments, d->slope_a, d->slope_b, d->level_q, d->resid_q2,
                                                   d->flat, d->site, d->candidates, d->summary, d->status};
  const size_t z[kReliefInputs + kReliefOutputs] = {sizeof(d2pc_sectors_ground_step), n * 4u, n * 8u, n * 8u, n * 8u * D2PC_SECTORS_SLOPE_MOMENTS, n,
                                                    n * 4u, n * 8u, n * 8u, n * 8u * D2PC_SECTORS_SLOPE_MOMENTS, n * 4u, n * 4u, n * 4u, n * 4u,
                                                    n, n, d->candidates ? size_t(d->n_candidates) * 8u : 0u, 16u, 16u};
  for (int i = 0; i < kReliefInputs + kReliefOutputs; ++i) bufs[i] = b[i], bytes[i] = z[i];
}

// what d2pc_sectors_relief_update_device refuses of a descriptor, for a session of plan `p` (the session adds the overlap
// with its own state: check_relief_state)
inline int check_relief_desc(const ReliefPlan &p, const d2pc_sectors_relief_desc *d, char *msg = nullptr, size_t msg_len = 0) {
  if (!d || d->struct_size != sizeof(d2pc_sectors_relief_desc)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_relief_desc");
  if (!d->step) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step is null");
  if (!d->frame_count || !d->frame_sum || !d->frame_sum2 || !d->frame_moments)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "frame_count, frame_sum, frame_sum2 and frame_moments are all required");
  if (!d->count && !d->sum && !d->sum2 && !d->moments && !d->slope_a && !d->slope_b && !d->level_q && !d->resid_q2 && !d->flat && !d->site &&
      !d->candidates && !d->summary && !d->status)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no output is given");
  if (d->candidates && (d->n_candidates < 1 || d->n_candidates > D2PC_SECTORS_GROUND_MAX_CANDIDATES))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "n_candidates of %d: 1 .. %d", d->n_candidates, D2PC_SECTORS_GROUND_MAX_CANDIDATES);
  if (misaligned(d->step, 4) || misaligned(d->frame_count, 4) || misaligned(d->count, 4) || misaligned(d->slope_a, 4) || misaligned(d->slope_b, 4) ||
      misaligned(d->level_q, 4) || misaligned(d->resid_q2, 4) || misaligned(d->summary, 4) || misaligned(d->status, 4))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step, frame_count or an output is not aligned to its type");
  if (misaligned(d->frame_sum, 8) || misaligned(d->frame_sum2, 8) || misaligned(d->frame_moments, 8) || misaligned(d->sum, 8) ||
      misaligned(d->sum2, 8) || misaligned(d->moments, 8) || misaligned(d->candidates, 8))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "frame_sum, frame_sum2, frame_moments, sum, sum2, moments and candidates must be 8-byte aligned");
  const void *bufs[kReliefInputs + kReliefOutputs];
  size_t bytes[kReliefInputs + kReliefOutputs];
  relief_buffers(p, d, bufs, bytes);
  for (int i = kReliefInputs; i < kReliefInputs + kReliefOutputs; ++i) {
    for (int k = 0; k < kReliefInputs; ++k)
      if (hulls_meet(bufs[i], bytes[i], bufs[k], bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "an output overlaps an input");
    for (int k = i + 1; k < kReliefInputs + kReliefOutputs; ++k)
      if (hulls_meet(bufs[i], bytes[i], bufs[k], bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "two outputs overlap");
  }
  return D2PC_OK;
}

// the session's own addition: nothing of an accepted descriptor lies inside the state block
inline int check_relief_state(const ReliefPlan &p, const d2pc_sectors_relief_desc *d, const void *state, char *msg = nullptr, size_t msg_len = 0) {
  const void *bufs[kReliefInputs + kReliefOutputs];
  size_t bytes[kReliefInputs + kReliefOutputs];
  relief_buffers(p, d, bufs, bytes);
  for (int i = 0; i < kReliefInputs + kReliefOutputs; ++i)
    if (hulls_meet(bufs[i], bytes[i], state, p.state_bytes)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a buffer overlaps the session's state");
  return D2PC_OK;
}

// One update as d2pc_sectors_relief.hip's kernels get it (d2pc_sectors_relief_capi.hip fills it).  The stream is a
// device-runtime stream handle.
struct ReliefLaunch {
  ReliefPlan plan;
  void *state;                 // DEVICE: the session's state block
  void *hand_on;               // DEVICE: the session's 14 bytes per cell between the two launches
  const d2pc_sectors_relief_desc *desc;   // HOST, accepted: the pointers are DEVICE
  void *stream;
};
// the runtime's error code as int
int launch_relief(const ReliefLaunch &a);
int launch_relief_reset(void *state, void *stream);

}  // namespace sectors
}  // namespace d2pc
