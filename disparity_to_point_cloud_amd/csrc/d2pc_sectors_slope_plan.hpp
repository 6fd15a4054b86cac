// d2pc_sectors_slope_plan.hpp -- the host side of the slope session of include/d2pc_sectors.h that needs no device: what a
// slope configuration and a slope descriptor are refused for, scale and max_tilt2, the LDS of a reducing block, the size of
// its slab and max_slope from an angle.  The grid's part is d2pc_sectors_ground_plan.hpp's (make_ground_plan, ground_blocks),
// the cloud part of a descriptor d2pc_sectors_plan.hpp's (check_cloud_given, check_cloud_sizes).
// Host code only and no HIP: plain g++ compiles it (tests/test_sectors_slope_cpu.py).
#pragma once
#include "d2pc_sectors_ground_plan.hpp"

namespace d2pc {
namespace sectors {

constexpr size_t kSlopeCellBytes = D2PC_SECTORS_SLOPE_CELL_BYTES;   // of a block's table and of its slab: nine 64-bit sums, the count
constexpr int kSlopeWords = 9;               // the 64-bit planes: sum, sum2, su, sw, suu, suw, sww, suk, swk
constexpr size_t kSlopeHandOnBytes = 14;     // per cell between the merge and the sites: count, level_q, resid_q2, flat, fitted
static_assert(kSlopeCellBytes == 8u * kSlopeWords + 4u, "a cell is its 64-bit planes and its count");
static_assert(size_t(D2PC_SECTORS_SLOPE_MAX_CELLS) * kSlopeCellBytes <= kLdsPerCu &&
                  size_t(D2PC_SECTORS_SLOPE_MAX_CELLS + 1) * kSlopeCellBytes > kLdsPerCu,
              "the largest grid is the largest table of one block's LDS");

struct SlopePlan {
  GroundPlan ground;           // lds_bytes, block_bytes and blocks_per_cu in it are the GROUND's: the slope's are below
  int sub;
  double scale, max_tilt2;
  size_t lds_bytes, block_bytes;
  int blocks_per_cu;
};

// D2PC_OK and *p filled, or the refusal (and its reason in msg, when given): first the ground configuration's, unchanged
inline int make_slope_plan(const d2pc_sectors_ground_config *g, const d2pc_sectors_slope_config *c, SlopePlan *p, char *msg = nullptr,
                           size_t msg_len = 0) {
  if (const int st = make_ground_plan(g, &p->ground, msg, msg_len)) return st;
  if (!c || c->struct_size != sizeof(d2pc_sectors_slope_config)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_slope_config");
  if (c->sub != 2 && c->sub != 4 && c->sub != 8 && c->sub != 16) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "sub of %d: 2, 4, 8 or 16", c->sub);
  if (!std::isfinite(c->max_slope) || !(c->max_slope >= 0.0f)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "max_slope must be finite and >= 0");
  for (int i = 0; i < 5; ++i)
    if (c->reserved[i]) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a reserved word is not zero");
  const size_t n = size_t(p->ground.n_cells);
  if (n * kSlopeCellBytes > kLdsPerCu)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "%d x %d cells: %d at the most (76 bytes each in one block's LDS)", p->ground.n_a, p->ground.n_b,
                        D2PC_SECTORS_SLOPE_MAX_CELLS);
  p->sub = c->sub;
  p->max_tilt2 = double(c->max_slope) * double(c->max_slope);
  p->scale = double(g->quantum) * double(2 * c->sub) / double(g->cell_size);
  p->lds_bytes = kSlopeCellBytes * n;
  p->block_bytes = 8u * size_t(kSlopeWords) * n + 8u * ((n + 1u) / 2u);   // (the slab after it stays 8-byte aligned for an odd n_cells)
  const size_t fit = kLdsPerCu / p->lds_bytes;
  p->blocks_per_cu = int(fit < size_t(kMaxBlocksPerCu) ? fit : size_t(kMaxBlocksPerCu));
  return D2PC_OK;
}

inline void fill_slope_geometry(const SlopePlan &p, d2pc_sectors_slope_geometry_t *g) {
  memset(g, 0, sizeof *g);
  g->n_cells = p.ground.n_cells, g->sub = p.sub;
  g->blocks_per_cu = p.blocks_per_cu;
  g->blocks = ground_blocks(p.ground.max_points, p.blocks_per_cu, kRefCus);
  g->lds_bytes = p.lds_bytes, g->block_bytes = p.block_bytes;
  g->device_bytes = size_t(g->blocks) * p.block_bytes + kSlopeHandOnBytes * size_t(p.ground.n_cells);
  g->scale = p.scale, g->max_tilt2 = p.max_tilt2;
}

// (float)tan(degrees * pi / 180) in double; 0 for an angle that gives none
inline float slope_of_degrees(double degrees) {
  if (!(degrees >= 0.0) || !(degrees < 90.0)) return 0.0f;
  return float(std::tan(degrees * 3.14159265358979323846 / 180.0));
}

// what d2pc_sectors_slope_process_device refuses of a descriptor, for a session of plan `p`: check_ground_desc's refusals in
// its order, with the slope's outputs beside the ground's
inline int check_slope_desc(const SlopePlan &p, const d2pc_sectors_slope_desc *d, char *msg = nullptr, size_t msg_len = 0) {
  if (!d || d->struct_size != sizeof(d2pc_sectors_slope_desc)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_slope_desc");
  if (const int st = check_cloud_given(*d, msg, msg_len)) return st;
  if (!d->step) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step is null");
  if (!d->count && !d->sum && !d->sum2 && !d->moments && !d->slope_a && !d->slope_b && !d->level_q && !d->resid_q2 && !d->flat && !d->site &&
      !d->candidates && !d->summary)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no output is given");
  if (d->candidates && (d->n_candidates < 1 || d->n_candidates > D2PC_SECTORS_GROUND_MAX_CANDIDATES))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "n_candidates of %d: 1 .. %d", d->n_candidates, D2PC_SECTORS_GROUND_MAX_CANDIDATES);
  if (misaligned(d->points, 16)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "points must be 16-byte aligned");
  if (misaligned(d->counts, 4) || misaligned(d->step, 4) || misaligned(d->count, 4) || misaligned(d->slope_a, 4) || misaligned(d->slope_b, 4) ||
      misaligned(d->level_q, 4) || misaligned(d->resid_q2, 4) || misaligned(d->summary, 4))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "counts, step or an output is not aligned to its type");
  if (misaligned(d->sum, 8) || misaligned(d->sum2, 8) || misaligned(d->moments, 8) || misaligned(d->candidates, 8))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "sum, sum2, moments and candidates must be 8-byte aligned");
  if (const int st = check_cloud_sizes(*d, msg, msg_len)) return st;
  const size_t n = size_t(p.ground.n_cells);
  const void *ins[4] = {d->points, d->counts, d->step, d->allowed};
  const size_t in_bytes[4] = {size_t(position_bound(*d) * uint64_t(d->point_step)), d->counts ? size_t(d->n_clouds) * 4u : 0u,
                              sizeof(d2pc_sectors_ground_step), n};
  const void *outs[12] = {d->count, d->sum, d->sum2, d->moments, d->slope_a, d->slope_b, d->level_q, d->resid_q2, d->flat, d->site,
                          d->candidates, d->summary};
  const size_t out_bytes[12] = {n * 4u, n * 8u, n * 8u, n * 8u * D2PC_SECTORS_SLOPE_MOMENTS, n * 4u, n * 4u, n * 4u, n * 4u, n, n,
                                d->candidates ? size_t(d->n_candidates) * 8u : 0u, 16u};
  for (int i = 0; i < 12; ++i) {
    for (int k = 0; k < 4; ++k)
      if (hulls_meet(outs[i], out_bytes[i], ins[k], in_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "an output overlaps an input");
    for (int k = i + 1; k < 12; ++k)
      if (hulls_meet(outs[i], out_bytes[i], outs[k], out_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "two outputs overlap");
  }
  return D2PC_OK;
}

// One call as d2pc_sectors_slope.hip's kernels get it (d2pc_sectors_slope_capi.hip fills it).  The stream is a hipStream_t.
struct SlopeLaunch {
  SlopePlan plan;
  CloudWalk walk;
  const void *step;            // DEVICE: d2pc_sectors_ground_step
  const uint8_t *allowed;
  void *slabs;                 // DEVICE: the session's blocks x plan.block_bytes
  void *hand_on;               // DEVICE: count, level_q, resid_q2 (4 bytes x n_cells each), then flat and fitted (n_cells each)
  uint32_t *count;
  int64_t *sum;
  uint64_t *sum2;
  int64_t *moments;
  float *slope_a, *slope_b;
  int32_t *level_q;
  uint32_t *resid_q2;
  uint8_t *flat, *site;
  void *candidates;
  uint32_t *summary;
  int n_candidates;            // 0 without candidates
  int blocks;                  // of this launch: min(the session's, shares)
  void *stream;
};
// hipError_t as int
int launch_slope(const SlopeLaunch &a);
int prepare_slope_kernels(const SlopePlan &p);   // once per session, on its device

}  // namespace sectors
}  // namespace d2pc
