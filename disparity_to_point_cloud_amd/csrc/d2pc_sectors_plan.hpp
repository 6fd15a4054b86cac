// d2pc_sectors_plan.hpp -- the host side of include/d2pc_sectors.h that needs no device: what a configuration and a
// descriptor are refused for, the constants the specification forms on the host (rmin2, rmax2, inv_h, the boundary
// tables) and the sizes of a block's tables.  Host code only and no HIP: plain g++ compiles it, and the checks run
// wherever the library loads (tests/test_sectors_cpu.py, tests/test_sectors_elevation_cpu.py, through
// d2pc_sectors_geometry / _table / _elevation_table / _desc_check).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/d2pc_sectors.h"

namespace d2pc {
namespace sectors {

constexpr int kThreads = 256;                                     // of a reducing block
constexpr int kPerLane = D2PC_SECTORS_SHARE_POINTS / kThreads;    // records a lane holds in flight
constexpr int kMaxBlocksPerCu = 4;
constexpr size_t kLdsPerCu = 160u * 1024u;                        // gfx950
constexpr int kRefCus = 256;                                      // MI355X: what geometry's device_bytes assumes
constexpr int kMaxCells = D2PC_SECTORS_MAX_SECTORS * D2PC_SECTORS_MAX_LAYERS;   // the largest table a block holds
constexpr float kHalfPi = 1.5707964f;                             // the float nearest pi / 2: an elevation band's bound
static_assert(kPerLane * kThreads == D2PC_SECTORS_SHARE_POINTS, "a share is a whole number of records per lane");

struct Plan {                // what the kernels get of a configuration
  int n_sectors, n_layers, n_cells, half;
  int layer_kind, elev;      // elev: entries of the elevation table, n_layers + 1; 0 for height layers
  float rmin2, rmax2, u_min, u_max, inv_h;
  int axis[3];               // 0, 1, 2: the coordinate picked for f, l, u
  uint32_t flip[3];          // 0x80000000 where the pick negates
  uint32_t min_count, no_obstacle_cm;
  size_t lds_bytes, block_bytes;
  int blocks_per_cu;
};

// (every refusal of this header and of d2pc_sectors_memory_plan.hpp: the status, and the reason in msg when given)
#define D2PC_SECTORS_REFUSE(st, ...) \
  do { if (msg) snprintf(msg, msg_len, __VA_ARGS__); return st; } while (0)

// D2PC_OK and *p filled, or the refusal (and its reason in msg, when given)
inline int make_plan(const d2pc_sectors_config *c, Plan *p, char *msg = nullptr, size_t msg_len = 0) {
  if (!c || c->struct_size != sizeof(d2pc_sectors_config)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_config");
  bool used[3] = {false, false, false};
  for (int i = 0; i < 3; ++i) {
    const int a = c->axes[i], m = a < 0 ? -a : a;
    if (a == INT32_MIN || m < 1 || m > 3 || used[m - 1])
      D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "axes {%d, %d, %d}: three of +-1, +-2, +-3 with distinct magnitudes", c->axes[0], c->axes[1], c->axes[2]);
    used[m - 1] = true;
    p->axis[i] = m - 1, p->flip[i] = a < 0 ? 0x80000000u : 0u;
  }
  if (c->n_sectors < 2 || c->n_sectors > D2PC_SECTORS_MAX_SECTORS || c->n_sectors % 2 != 0)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "n_sectors of %d: even, 2 .. %d", c->n_sectors, D2PC_SECTORS_MAX_SECTORS);
  if (!std::isfinite(c->azimuth0)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "azimuth0 is not finite");
  if (std::isnan(c->r_min) || std::isnan(c->r_max) || std::isnan(c->u_min) || std::isnan(c->u_max))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a NaN gate");
  if (c->r_min < 0.0f || c->r_min > c->r_max) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "the range gate needs 0 <= r_min <= r_max");
  if (c->u_min > c->u_max) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "u_min > u_max");
  if (c->min_count < 1) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "min_count of %d", c->min_count);
  if (c->no_obstacle_cm > 65535u) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no_obstacle_cm of %u does not fit 16 bits", c->no_obstacle_cm);
  // (after every other INVALID_ARG and before the first BAD_SIZE: no status of a height-mode configuration moves)
  if (c->layer_kind != D2PC_SECTORS_LAYERS_HEIGHT && c->layer_kind != D2PC_SECTORS_LAYERS_ELEVATION)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "layer_kind of %d: 0 (height) or 1 (elevation)", c->layer_kind);
  p->layer_kind = c->layer_kind, p->elev = 0;
  p->inv_h = 0.0f;
  if (c->layer_kind == D2PC_SECTORS_LAYERS_ELEVATION) {
    if (c->n_layers < 1 || c->n_layers > D2PC_SECTORS_MAX_ELEVATION_LAYERS)
      D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "n_layers of %d: 1 .. %d elevation layers", c->n_layers, D2PC_SECTORS_MAX_ELEVATION_LAYERS);
    if (c->n_sectors * c->n_layers > kMaxCells)
      D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "%d x %d cells: %d at the most", c->n_sectors, c->n_layers, kMaxCells);
    if (!(c->u_min >= -kHalfPi) || !(c->u_max <= kHalfPi))   // (infinities included)
      D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "the elevation band must lie within -+1.5707964 rad");
    if (c->u_min == c->u_max) D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "the elevation band is empty");
    p->elev = c->n_layers + 1;
  } else if (c->n_layers < 1 || c->n_layers > D2PC_SECTORS_MAX_LAYERS) {
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "n_layers of %d: 1 .. %d", c->n_layers, D2PC_SECTORS_MAX_LAYERS);
  } else if (c->n_layers > 1) {
    if (!std::isfinite(c->u_min) || !std::isfinite(c->u_max) || !(c->u_min < c->u_max))
      D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "%d layers need a finite height band with u_min < u_max", c->n_layers);
    p->inv_h = float(double(c->n_layers) / (double(c->u_max) - double(c->u_min)));
    if (!std::isfinite(p->inv_h) || !(p->inv_h > 0.0f))
      D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "the height band gives no finite slab height in float32");
  }
  p->n_sectors = c->n_sectors, p->n_layers = c->n_layers, p->n_cells = c->n_sectors * c->n_layers, p->half = c->n_sectors / 2;
  {
    // (a float product is rounded once whatever the contraction mode; volatile keeps x87-style excess precision out)
    volatile float a = c->r_min * c->r_min, b = c->r_max * c->r_max;
    p->rmin2 = a, p->rmax2 = b;
  }
  p->u_min = c->u_min, p->u_max = c->u_max;
  p->min_count = uint32_t(c->min_count), p->no_obstacle_cm = c->no_obstacle_cm;
  // LDS of a block: 8-byte keys, 4-byte counts, then the table's (c, s) pairs, then the elevation table's
  p->lds_bytes = size_t(p->n_cells) * 12u + size_t(p->half) * 8u + size_t(p->elev) * 8u;
  p->block_bytes = size_t(p->n_cells) * 12u;
  const size_t fit = kLdsPerCu / p->lds_bytes;
  p->blocks_per_cu = int(fit < size_t(kMaxBlocksPerCu) ? fit : size_t(kMaxBlocksPerCu));
  return D2PC_OK;
}

inline void fill_geometry(const Plan &p, d2pc_sectors_geometry_t *g) {
  memset(g, 0, sizeof *g);
  g->n_cells = p.n_cells, g->table_entries = p.half;
  g->rmin2 = p.rmin2, g->rmax2 = p.rmax2, g->inv_h = p.inv_h;
  g->share_points = D2PC_SECTORS_SHARE_POINTS;
  g->blocks_per_cu = p.blocks_per_cu;
  g->elevation_entries = p.elev;
  g->lds_bytes = p.lds_bytes, g->block_bytes = p.block_bytes;
  g->device_bytes = size_t(p.blocks_per_cu) * size_t(kRefCus) * p.block_bytes + size_t(p.half) * 8u + size_t(p.elev) * 8u;
}

// c_j, s_j: the angle and its cosine and sine in double, rounded to float once
inline void fill_table(const d2pc_sectors_config &c, float *cs, float *sn) {
  const double two_pi = 6.283185307179586476925286766559;
  for (int j = 0; j < c.n_sectors / 2; ++j) {
    const double a = c.azimuth0 + two_pi * double(j) / double(c.n_sectors);
    cs[j] = float(std::cos(a)), sn[j] = float(std::sin(a));
  }
}

// ce_i, se_i of an elevation-mode configuration: the boundary elevation and its cosine and sine in double, rounded once
inline void fill_elevation_table(const d2pc_sectors_config &c, float *ce, float *se) {
  const double lo = double(c.u_min), span = double(c.u_max) - double(c.u_min);
  for (int i = 0; i <= c.n_layers; ++i) {
    const double e = lo + (double(i) * span) / double(c.n_layers);
    ce[i] = float(std::cos(e)), se[i] = float(std::sin(e));
  }
}

inline bool hulls_meet(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
  if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

inline bool misaligned(const void *q, size_t to) { return reinterpret_cast<uintptr_t>(q) % to != 0; }

// The cloud part of a descriptor of either kind (the sectors' or the memory's), in the two runs its refusals come in: a
// descriptor's own null and alignment refusals, and the alignment of `points` between those, lie between the runs
template <class Desc>
inline int check_cloud_given(const Desc &d, char *msg, size_t msg_len) {
  if (d.point_step != 16 && d.point_step != 32) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "point_step of %d: 16 or 32", d.point_step);
  if (d.n_clouds < 1 || d.n_clouds > 65535) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "n_clouds of %d: 1 .. 65,535", d.n_clouds);
  if (!d.points) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "points is null");
  return D2PC_OK;
}
template <class Desc>
inline int check_cloud_sizes(const Desc &d, char *msg, size_t msg_len) {
  const uint64_t cp = d.cloud_points;
  if (cp == 0 || cp >= (uint64_t(1) << 32)) D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "cloud_points of %zu: 1 .. 2^32 - 1", d.cloud_points);
  const uint64_t stride = d.n_clouds > 1 ? uint64_t(d.points_frame_stride_points) : 0;
  if (d.n_clouds > 1 && stride < cp) D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "the frame stride is smaller than cloud_points (%zu)", d.cloud_points);
  // (n_clouds - 1) * stride + cloud_points - 1 <= 0xFFFFFFFE, formed so that nothing wraps
  const uint64_t room = 0xFFFFFFFFull - cp;
  if (d.n_clouds > 1 && stride > room / uint64_t(d.n_clouds - 1))
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "the position of the last record does not fit below 0xFFFFFFFF");
  return D2PC_OK;
}

// (n_clouds - 1) * stride + cloud_points of a checked descriptor of either kind: positions below it are records of `points`
template <class Desc>
inline uint64_t position_bound(const Desc &d) {
  const uint64_t stride = d.n_clouds > 1 ? uint64_t(d.points_frame_stride_points) : 0;
  return uint64_t(d.n_clouds - 1) * stride + uint64_t(d.cloud_points);
}

// The records of a call as shares of D2PC_SECTORS_SHARE_POINTS records of one cloud each: what the reducing kernels of the
// grid and of the ground walk (load_share, d2pc_sectors_device.hpp), and what their launches and kernel arguments embed
struct CloudWalk {
  const void *points;
  const uint32_t *counts;
  uint64_t stride;             // records between the clouds; 0 for one cloud
  uint64_t shares;             // n_clouds * shares_per_cloud
  uint32_t shares_per_cloud, cloud_points, n_clouds, step16;  // step16: 16-byte units of a record
};

// the walk over the cloud of a checked descriptor of either kind
template <class Desc>
inline CloudWalk cloud_walk(const Desc &d) {
  CloudWalk w;
  w.points = d.points, w.counts = d.counts;
  w.stride = d.n_clouds > 1 ? uint64_t(d.points_frame_stride_points) : 0;
  w.cloud_points = uint32_t(d.cloud_points), w.n_clouds = uint32_t(d.n_clouds), w.step16 = uint32_t(d.point_step / 16);
  w.shares_per_cloud = uint32_t((uint64_t(d.cloud_points) + D2PC_SECTORS_SHARE_POINTS - 1) / D2PC_SECTORS_SHARE_POINTS);
  w.shares = uint64_t(w.shares_per_cloud) * uint64_t(w.n_clouds);
  return w;
}

// what d2pc_sectors_process_device refuses of a descriptor, for a session of plan `p`
inline int check_desc(const Plan &p, const d2pc_sectors_desc *d, char *msg = nullptr, size_t msg_len = 0) {
  if (!d || d->struct_size != sizeof(d2pc_sectors_desc)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_desc");
  if (const int st = check_cloud_given(*d, msg, msg_len)) return st;
  if (!d->range && !d->count && !d->nearest && !d->distance_cm) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no output is given");
  if (misaligned(d->points, 16)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "points must be 16-byte aligned");
  if (misaligned(d->counts, 4) || misaligned(d->range, 4) || misaligned(d->count, 4) || misaligned(d->nearest, 4) ||
      misaligned(d->distance_cm, 2))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "counts or an output is not aligned to its type");
  if (const int st = check_cloud_sizes(*d, msg, msg_len)) return st;
  const size_t in_bytes = size_t(position_bound(*d) * uint64_t(d->point_step));
  const size_t cnt_bytes = d->counts ? size_t(d->n_clouds) * 4u : 0;
  const size_t n = size_t(p.n_cells);
  const void *outs[4] = {d->range, d->count, d->nearest, d->distance_cm};
  const size_t out_bytes[4] = {n * 4u, n * 4u, n * 4u, n * 2u};
  for (int i = 0; i < 4; ++i) {
    if (hulls_meet(outs[i], out_bytes[i], d->points, in_bytes) || hulls_meet(outs[i], out_bytes[i], d->counts, cnt_bytes))
      D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "an output overlaps points or counts");
    for (int k = i + 1; k < 4; ++k)
      if (hulls_meet(outs[i], out_bytes[i], outs[k], out_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "two outputs overlap");
  }
  return D2PC_OK;
}

// One call as d2pc_sectors.hip's kernels get it (d2pc_sectors_capi.hip fills it).  The stream is a hipStream_t.
struct Launch {
  Plan plan;
  CloudWalk walk;
  const float *table;          // DEVICE: half x (c, s), then plan.elev x (ce, se)
  uint64_t *slab_keys;         // DEVICE: blocks x n_cells
  uint32_t *slab_counts;       // DEVICE: blocks x n_cells
  float *range;
  uint32_t *count, *nearest;
  uint16_t *distance_cm;
  int blocks;
  void *stream;
};
// hipError_t as int
int launch_sectors(const Launch &a);
int prepare_sectors_kernels(const Plan &p);      // once per session, on its device

}  // namespace sectors
}  // namespace d2pc
