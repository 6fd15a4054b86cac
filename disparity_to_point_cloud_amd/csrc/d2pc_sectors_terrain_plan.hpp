// d2pc_sectors_terrain_plan.hpp -- the host side of the terrain session of include/d2pc_sectors.h that needs no device: what
// a terrain configuration and a terrain descriptor are refused for, and the sizes of the state block (16 headers, then
// `depth` tables in the ground slab's order).  The grid's part is d2pc_sectors_ground_plan.hpp's (make_ground_plan).
// Host code only and no device runtime: plain g++ compiles it (tests/test_sectors_terrain_cpu.py,
// tests/cpp/sectors_terrain_plan_main.cpp).
#pragma once
#include "d2pc_sectors_ground_plan.hpp"

namespace d2pc {
namespace sectors {

constexpr size_t kTerrainHeaderBytes = 16;   // {int32 ia0, int32 jb0, float h0, uint32 seq}
constexpr size_t kTerrainHeadersBytes = kTerrainHeaderBytes * D2PC_SECTORS_TERRAIN_MAX_DEPTH;
constexpr float kTerrainAnchorMax = 536870912.0f;   // 2^29: the largest |corner| in cells

struct TerrainPlan {
  GroundPlan ground;
  int depth;
  size_t slot_bytes;    // 20 bytes per cell, rounded up to a multiple of 16
  size_t state_bytes;   // the headers and `depth` tables
};

// D2PC_OK and *p filled, or the refusal (and its reason in msg, when given): first the ground configuration's, unchanged
inline int make_terrain_plan(const d2pc_sectors_ground_config *g, const d2pc_sectors_terrain_config *c, TerrainPlan *p, char *msg = nullptr,
                             size_t msg_len = 0) {
  if (const int st = make_ground_plan(g, &p->ground, msg, msg_len)) return st;
  if (!c || c->struct_size != sizeof(d2pc_sectors_terrain_config)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_terrain_config");
  if (c->depth < 1 || c->depth > D2PC_SECTORS_TERRAIN_MAX_DEPTH)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "depth of %d: 1 .. %d", c->depth, D2PC_SECTORS_TERRAIN_MAX_DEPTH);
  for (int i = 0; i < 6; ++i)
    if (c->reserved[i]) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a reserved word is not zero");
  p->depth = c->depth;
  p->slot_bytes = (kGroundCellBytes * size_t(p->ground.n_cells) + 15u) / 16u * 16u;
  p->state_bytes = kTerrainHeadersBytes + size_t(p->depth) * p->slot_bytes;
  return D2PC_OK;
}

inline void fill_terrain_geometry(const TerrainPlan &p, d2pc_sectors_terrain_geometry_t *g) {
  memset(g, 0, sizeof *g);
  g->n_cells = p.ground.n_cells, g->inv_c = p.ground.inv_c;
  g->slot_bytes = p.slot_bytes, g->state_bytes = p.state_bytes;
  g->headers_offset = 0, g->tables_offset = kTerrainHeadersBytes;
}

// what d2pc_sectors_terrain_update_device refuses of a descriptor, for a session of plan `p` (the session adds the overlap
// with its own state: check_terrain_state)
inline int check_terrain_desc(const TerrainPlan &p, const d2pc_sectors_terrain_desc *d, char *msg = nullptr, size_t msg_len = 0) {
  if (!d || d->struct_size != sizeof(d2pc_sectors_terrain_desc)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_terrain_desc");
  if (!d->step) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step is null");
  if (!d->frame_count || !d->frame_sum || !d->frame_sum2) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "frame_count, frame_sum and frame_sum2 are all required");
  if (!d->count && !d->sum && !d->sum2 && !d->mean_q && !d->spread_q2 && !d->flat && !d->site && !d->candidates && !d->summary && !d->status)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no output is given");
  if (d->candidates && (d->n_candidates < 1 || d->n_candidates > D2PC_SECTORS_GROUND_MAX_CANDIDATES))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "n_candidates of %d: 1 .. %d", d->n_candidates, D2PC_SECTORS_GROUND_MAX_CANDIDATES);
  if (misaligned(d->step, 4) || misaligned(d->frame_count, 4) || misaligned(d->count, 4) || misaligned(d->mean_q, 4) ||
      misaligned(d->spread_q2, 4) || misaligned(d->summary, 4) || misaligned(d->status, 4))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step, frame_count or an output is not aligned to its type");
  if (misaligned(d->frame_sum, 8) || misaligned(d->frame_sum2, 8) || misaligned(d->sum, 8) || misaligned(d->sum2, 8) || misaligned(d->candidates, 8))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "frame_sum, frame_sum2, sum, sum2 and candidates must be 8-byte aligned");
  const size_t n = size_t(p.ground.n_cells);
  const void *ins[5] = {d->step, d->frame_count, d->frame_sum, d->frame_sum2, d->allowed};
  const size_t in_bytes[5] = {sizeof(d2pc_sectors_ground_step), n * 4u, n * 8u, n * 8u, n};
  const void *outs[10] = {d->count, d->sum, d->sum2, d->mean_q, d->spread_q2, d->flat, d->site, d->candidates, d->summary, d->status};
  const size_t out_bytes[10] = {n * 4u, n * 8u, n * 8u, n * 4u, n * 4u, n, n, d->candidates ? size_t(d->n_candidates) * 8u : 0u, 16u, 16u};
  for (int i = 0; i < 10; ++i) {
    for (int k = 0; k < 5; ++k)
      if (hulls_meet(outs[i], out_bytes[i], ins[k], in_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "an output overlaps an input");
    for (int k = i + 1; k < 10; ++k)
      if (hulls_meet(outs[i], out_bytes[i], outs[k], out_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "two outputs overlap");
  }
  return D2PC_OK;
}

// the session's own addition: nothing of an accepted descriptor lies inside the state block
inline int check_terrain_state(const TerrainPlan &p, const d2pc_sectors_terrain_desc *d, const void *state, char *msg = nullptr, size_t msg_len = 0) {
  const size_t n = size_t(p.ground.n_cells);
  const void *bufs[15] = {d->step, d->frame_count, d->frame_sum, d->frame_sum2, d->allowed, d->count, d->sum, d->sum2, d->mean_q, d->spread_q2,
                          d->flat, d->site, d->candidates, d->summary, d->status};
  const size_t bytes[15] = {sizeof(d2pc_sectors_ground_step), n * 4u, n * 8u, n * 8u, n, n * 4u, n * 8u, n * 8u, n * 4u, n * 4u, n, n,
                            d->candidates ? size_t(d->n_candidates) * 8u : 0u, 16u, 16u};
  for (int i = 0; i < 15; ++i)
    if (hulls_meet(bufs[i], bytes[i], state, p.state_bytes)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a buffer overlaps the session's state");
  return D2PC_OK;
}

// One update as d2pc_sectors_terrain.hip's kernel gets it (d2pc_sectors_terrain_capi.hip fills it).  The stream is a
// device-runtime stream handle.
struct TerrainLaunch {
  TerrainPlan plan;
  void *state;                 // DEVICE: the session's state block
  const void *step;            // DEVICE: d2pc_sectors_ground_step
  const uint32_t *frame_count;
  const int64_t *frame_sum;
  const uint64_t *frame_sum2;
  const uint8_t *allowed;
  uint32_t *count;
  int64_t *sum;
  uint64_t *sum2;
  int32_t *mean_q;
  uint32_t *spread_q2;
  uint8_t *flat, *site;
  void *candidates;
  uint32_t *summary, *status;
  int n_candidates;            // 0 without candidates
  void *stream;
};
// the runtime's error code as int
int launch_terrain(const TerrainLaunch &a);
int launch_terrain_reset(void *state, void *stream);

}  // namespace sectors
}  // namespace d2pc
