// d2pc_sectors_ground_plan.hpp -- the host side of the ground session of include/d2pc_sectors.h that needs no device: what a
// ground configuration and a ground descriptor are refused for, inv_c and inv_q, max_spread_q2 from a standard deviation,
// the LDS of a reducing block and the number of blocks a session holds slabs for.  The cloud part of a descriptor is
// d2pc_sectors_plan.hpp's (check_cloud_given, check_cloud_sizes).
// Host code only and no HIP: plain g++ compiles it (tests/test_sectors_ground_cpu.py, tests/cpp/sectors_ground_plan_main.cpp).
#pragma once
#include "d2pc_sectors_plan.hpp"

namespace d2pc {
namespace sectors {

constexpr int kGroundMaxCells = D2PC_SECTORS_GROUND_MAX_CELLS_PER_AXIS * D2PC_SECTORS_GROUND_MAX_CELLS_PER_AXIS;
constexpr size_t kGroundCellBytes = 20;      // of a block's table and of its slab: sum (8), sum2 (8), count (4)
constexpr size_t kGroundHandOnBytes = 13;    // per cell between the merge and the sites: count, mean_q, spread_q2, flat
constexpr int kGroundSharesPerBlock = 4;     // shares of max_points a reducing block is sized for
constexpr int kGroundSiteThreads = 1024;     // the one block of the sites
constexpr int kGroundSiteWaves = kGroundSiteThreads / 64;
constexpr int kGroundPerLane = kGroundMaxCells / kGroundSiteThreads;   // cells a lane of it holds: 4
constexpr int kGroundMergeCells = 16, kGroundMergeSlices = 16;         // the merging block is cells x slices of the slabs
static_assert(kGroundPerLane * kGroundSiteThreads == kGroundMaxCells, "a lane's cells cover the largest grid");
static_assert(kGroundMergeCells * kGroundMergeSlices == kThreads, "the merging block is cells x slices");

struct GroundPlan {
  int n_a, n_b, n_cells;
  int axis[3];               // 0, 1, 2: the world coordinate picked for a, b, h
  uint32_t flip[3];          // 0x80000000 where the pick negates
  float inv_c, inv_q;
  uint32_t min_count, max_spread_q2, max_step_q, w_dist, w_rough, rough_cap, max_points;
  int window;
  size_t lds_bytes, block_bytes;
  int blocks_per_cu;
};

// what the site stage (d2pc_sectors_ground_sites.hpp) reads of a plan: the ground's and the terrain's kernel arguments embed it
struct GroundSiteGrid {
  int n_a, n_b, n_cells, window;
  uint32_t max_step_q, w_dist, w_rough, rough_cap;
};

inline GroundSiteGrid ground_site_grid(const GroundPlan &p) {
  GroundSiteGrid g;
  g.n_a = p.n_a, g.n_b = p.n_b, g.n_cells = p.n_cells, g.window = p.window;
  g.max_step_q = p.max_step_q, g.w_dist = p.w_dist, g.w_rough = p.w_rough, g.rough_cap = p.rough_cap;
  return g;
}

// reducing blocks of a session on a device of `cus` compute units: one per kGroundSharesPerBlock shares of max_points,
// 1 .. blocks_per_cu x cus; all of them for max_points 0
inline int ground_blocks(uint32_t max_points, int blocks_per_cu, int cus) {
  const uint64_t most = uint64_t(blocks_per_cu) * uint64_t(cus < 1 ? 1 : cus);
  if (max_points == 0) return int(most);
  const uint64_t shares = (uint64_t(max_points) + D2PC_SECTORS_SHARE_POINTS - 1) / D2PC_SECTORS_SHARE_POINTS;
  const uint64_t want = (shares + kGroundSharesPerBlock - 1) / kGroundSharesPerBlock;
  return int(want < 1 ? 1 : (want > most ? most : want));
}

// D2PC_OK and *p filled, or the refusal (and its reason in msg, when given): every INVALID_ARG before the first BAD_SIZE
inline int make_ground_plan(const d2pc_sectors_ground_config *c, GroundPlan *p, char *msg = nullptr, size_t msg_len = 0) {
  if (!c || c->struct_size != sizeof(d2pc_sectors_ground_config)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_ground_config");
  bool used[3] = {false, false, false};
  for (int i = 0; i < 3; ++i) {
    const int a = c->axes[i], m = a < -3 || a > 3 ? 0 : (a < 0 ? -a : a);   // (INT32_MIN has no negation)
    if (m < 1 || used[m - 1])
      D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "axes {%d, %d, %d}: three of +-1, +-2, +-3 with distinct magnitudes", c->axes[0], c->axes[1], c->axes[2]);
    used[m - 1] = true;
    p->axis[i] = m - 1, p->flip[i] = a < 0 ? 0x80000000u : 0u;
  }
  if (!std::isfinite(c->cell_size) || !(c->cell_size > 0.0f)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "cell_size must be finite and > 0");
  if (!std::isfinite(c->quantum) || !(c->quantum > 0.0f)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "quantum must be finite and > 0");
  if (c->min_count < 1u) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "min_count of 0");
  if (c->max_step_q > 65535u) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "max_step_q of %u does not fit 16 bits", c->max_step_q);
  if (c->w_dist > D2PC_SECTORS_GROUND_MAX_WEIGHT || c->w_rough > D2PC_SECTORS_GROUND_MAX_WEIGHT)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "weights of %u / %u: %d at the most", c->w_dist, c->w_rough, D2PC_SECTORS_GROUND_MAX_WEIGHT);
  if (c->rough_cap > 65535u) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "rough_cap of %u does not fit 16 bits", c->rough_cap);
  if (c->reserved[0] || c->reserved[1] || c->reserved[2]) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a reserved word is not zero");
  if (c->n_a < 2 || c->n_a > D2PC_SECTORS_GROUND_MAX_CELLS_PER_AXIS || c->n_b < 2 || c->n_b > D2PC_SECTORS_GROUND_MAX_CELLS_PER_AXIS)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "%d x %d cells: 2 .. %d each", c->n_a, c->n_b, D2PC_SECTORS_GROUND_MAX_CELLS_PER_AXIS);
  if (c->window < 0 || c->window > D2PC_SECTORS_GROUND_MAX_WINDOW)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "window of %d: 0 .. %d", c->window, D2PC_SECTORS_GROUND_MAX_WINDOW);
  p->inv_c = float(1.0 / double(c->cell_size)), p->inv_q = float(1.0 / double(c->quantum));
  if (!std::isfinite(p->inv_c) || !(p->inv_c > 0.0f)) D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "cell_size gives no positive finite inverse in float32");
  if (!std::isfinite(p->inv_q) || !(p->inv_q > 0.0f)) D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "quantum gives no positive finite inverse in float32");
  p->n_a = c->n_a, p->n_b = c->n_b, p->n_cells = c->n_a * c->n_b;
  p->min_count = c->min_count, p->max_spread_q2 = c->max_spread_q2, p->max_step_q = c->max_step_q;
  p->w_dist = c->w_dist, p->w_rough = c->w_rough, p->rough_cap = c->rough_cap, p->max_points = c->max_points;
  p->window = c->window;
  p->lds_bytes = kGroundCellBytes * size_t(p->n_cells);
  p->block_bytes = 16u * size_t(p->n_cells) + 8u * ((size_t(p->n_cells) + 1u) / 2u);   // (the slab after it stays 8-byte aligned for an odd n_cells)
  const size_t fit = kLdsPerCu / p->lds_bytes;
  p->blocks_per_cu = int(fit < size_t(kMaxBlocksPerCu) ? fit : size_t(kMaxBlocksPerCu));
  return D2PC_OK;
}

inline void fill_ground_geometry(const GroundPlan &p, d2pc_sectors_ground_geometry_t *g) {
  memset(g, 0, sizeof *g);
  g->n_cells = p.n_cells, g->inv_c = p.inv_c, g->inv_q = p.inv_q;
  g->share_points = D2PC_SECTORS_SHARE_POINTS;
  g->blocks_per_cu = p.blocks_per_cu;
  g->blocks = ground_blocks(p.max_points, p.blocks_per_cu, kRefCus);
  g->lds_bytes = p.lds_bytes, g->block_bytes = p.block_bytes;
  g->device_bytes = size_t(g->blocks) * p.block_bytes + kGroundHandOnBytes * size_t(p.n_cells);
}

// floor((std / quantum)^2) in double, clamped to 0xFFFFFFFE; 0 for arguments that give none
inline uint32_t ground_spread_of_std(double quantum, double std_dev) {
  if (!std::isfinite(quantum) || !(quantum > 0.0) || !(std_dev >= 0.0)) return 0u;
  const double r = std_dev / quantum, q = std::floor(r * r);
  return q >= 4294967294.0 ? 0xFFFFFFFEu : uint32_t(q);   // (an infinite std_dev included)
}

// what d2pc_sectors_ground_process_device refuses of a descriptor, for a session of plan `p`
inline int check_ground_desc(const GroundPlan &p, const d2pc_sectors_ground_desc *d, char *msg = nullptr, size_t msg_len = 0) {
  if (!d || d->struct_size != sizeof(d2pc_sectors_ground_desc)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_ground_desc");
  if (const int st = check_cloud_given(*d, msg, msg_len)) return st;
  if (!d->step) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step is null");
  if (!d->count && !d->sum && !d->sum2 && !d->mean_q && !d->spread_q2 && !d->flat && !d->site && !d->candidates && !d->summary)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no output is given");
  if (d->candidates && (d->n_candidates < 1 || d->n_candidates > D2PC_SECTORS_GROUND_MAX_CANDIDATES))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "n_candidates of %d: 1 .. %d", d->n_candidates, D2PC_SECTORS_GROUND_MAX_CANDIDATES);
  if (misaligned(d->points, 16)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "points must be 16-byte aligned");
  if (misaligned(d->counts, 4) || misaligned(d->step, 4) || misaligned(d->count, 4) || misaligned(d->mean_q, 4) ||
      misaligned(d->spread_q2, 4) || misaligned(d->summary, 4))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "counts, step or an output is not aligned to its type");
  if (misaligned(d->sum, 8) || misaligned(d->sum2, 8) || misaligned(d->candidates, 8))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "sum, sum2 and candidates must be 8-byte aligned");
  if (const int st = check_cloud_sizes(*d, msg, msg_len)) return st;
  const size_t n = size_t(p.n_cells);
  const void *ins[4] = {d->points, d->counts, d->step, d->allowed};
  const size_t in_bytes[4] = {size_t(position_bound(*d) * uint64_t(d->point_step)), d->counts ? size_t(d->n_clouds) * 4u : 0u,
                              sizeof(d2pc_sectors_ground_step), n};
  const void *outs[9] = {d->count, d->sum, d->sum2, d->mean_q, d->spread_q2, d->flat, d->site, d->candidates, d->summary};
  const size_t out_bytes[9] = {n * 4u, n * 8u, n * 8u, n * 4u, n * 4u, n, n, d->candidates ? size_t(d->n_candidates) * 8u : 0u, 16u};
  for (int i = 0; i < 9; ++i) {
    for (int k = 0; k < 4; ++k)
      if (hulls_meet(outs[i], out_bytes[i], ins[k], in_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "an output overlaps an input");
    for (int k = i + 1; k < 9; ++k)
      if (hulls_meet(outs[i], out_bytes[i], outs[k], out_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "two outputs overlap");
  }
  return D2PC_OK;
}

// One call as d2pc_sectors_ground.hip's kernels get it (d2pc_sectors_ground_capi.hip fills it).  The stream is a hipStream_t.
struct GroundLaunch {
  GroundPlan plan;
  CloudWalk walk;
  const void *step;            // DEVICE: d2pc_sectors_ground_step
  const uint8_t *allowed;
  void *slabs;                 // DEVICE: the session's blocks x (sum, sum2, count of n_cells each)
  void *hand_on;               // DEVICE: count, mean_q, spread_q2 (4 bytes x n_cells each), then flat (n_cells)
  uint32_t *count;
  int64_t *sum;
  uint64_t *sum2;
  int32_t *mean_q;
  uint32_t *spread_q2;
  uint8_t *flat, *site;
  void *candidates;
  uint32_t *summary;
  int n_candidates;            // 0 without candidates
  int blocks;                  // of this launch: min(the session's, shares)
  void *stream;
};
// hipError_t as int
int launch_ground(const GroundLaunch &a);
int prepare_ground_kernels(const GroundPlan &p);   // once per session, on its device

}  // namespace sectors
}  // namespace d2pc
