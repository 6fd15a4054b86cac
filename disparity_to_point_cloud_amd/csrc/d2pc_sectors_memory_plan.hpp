// d2pc_sectors_memory_plan.hpp -- the host side of the memory session of include/d2pc_sectors.h that needs no device:
// what a memory configuration and a memory descriptor are refused for, the LDS of the one block and the coverage of the
// cells by the cameras' fields of view.  The grid's own refusals, constants and tables, the refusals of a descriptor's
// cloud part and the position bound are d2pc_sectors_plan.hpp's (make_plan, fill_table, fill_elevation_table,
// check_cloud_given / _sizes, position_bound).  Host code only and no HIP: plain g++ compiles
// it (tests/test_sectors_memory_cpu.py, tests/cpp/sectors_memory_plan_main.cpp).
#pragma once
#include "d2pc_sectors_plan.hpp"

namespace d2pc {
namespace sectors {

constexpr int kMemoryThreads = 1024;     // the one block of an update
constexpr int kMemoryPerLane = 3;        // remembered records a lane re-bins per pass: one table read serves them
constexpr uint32_t kEmptyAge = 0xFFFFFFFFu;   // the age word of an empty record
constexpr uint32_t kOldestAge = 0xFFFFFFFEu;  // where an age saturates

struct MemoryPlan {
  Plan grid;
  uint32_t max_age;
  size_t lds_bytes;          // the carry keys (8 bytes a cell), then the azimuth and the elevation table
};

// D2PC_OK and *p filled, or the refusal: the grid's, as make_plan makes them, then the memory's own
inline int make_memory_plan(const d2pc_sectors_config *grid, const d2pc_sectors_memory_config *m, MemoryPlan *p, char *msg = nullptr,
                            size_t msg_len = 0) {
  const int st = make_plan(grid, &p->grid, msg, msg_len);
  if (st != D2PC_OK) return st;
  if (!m || m->struct_size != sizeof(d2pc_sectors_memory_config)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_memory_config");
  if (m->max_age > kOldestAge) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "max_age of 0x%x: 0xFFFFFFFE at the most", m->max_age);
  p->max_age = m->max_age;
  p->lds_bytes = size_t(p->grid.n_cells) * 8u + size_t(p->grid.half) * 8u + size_t(p->grid.elev) * 8u;
  return D2PC_OK;
}

// what d2pc_sectors_memory_update_device refuses of a descriptor, for a session of plan `p`
inline int check_memory_desc(const MemoryPlan &p, const d2pc_sectors_memory_desc *d, char *msg = nullptr, size_t msg_len = 0) {
  if (!d || d->struct_size != sizeof(d2pc_sectors_memory_desc)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_memory_desc");
  if (const int st = check_cloud_given(*d, msg, msg_len)) return st;
  if (!d->count || !d->nearest) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "count or nearest is null");
  if (!d->step) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step is null");
  if (!d->range && !d->distance_cm && !d->age && !d->records) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no output is given");
  if (misaligned(d->points, 16)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "points must be 16-byte aligned");
  if (misaligned(d->records, 16)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "records must be 16-byte aligned");
  if (misaligned(d->count, 4) || misaligned(d->nearest, 4) || misaligned(d->step, 4) || misaligned(d->range, 4) ||
      misaligned(d->age, 4) || misaligned(d->distance_cm, 2))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "count, nearest, step or an output is not aligned to its type");
  if (const int st = check_cloud_sizes(*d, msg, msg_len)) return st;
  const size_t n = size_t(p.grid.n_cells);
  const void *ins[5] = {d->points, d->count, d->nearest, d->step, d->covered};
  const size_t in_bytes[5] = {size_t(position_bound(*d) * uint64_t(d->point_step)), n * 4u, n * 4u, sizeof(d2pc_sectors_memory_step), n};
  const void *outs[4] = {d->range, d->distance_cm, d->age, d->records};
  const size_t out_bytes[4] = {n * 4u, n * 2u, n * 4u, n * 16u};
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 5; ++k)
      if (hulls_meet(outs[i], out_bytes[i], ins[k], in_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "an output overlaps an input");
    for (int k = i + 1; k < 4; ++k)
      if (hulls_meet(outs[i], out_bytes[i], outs[k], out_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "two outputs overlap");
  }
  return D2PC_OK;
}

// covered[cell] = 1 where the cell's centre direction lies inside some field of view, all in double (d2pc_sectors.h)
inline void fill_coverage(const d2pc_sectors_config &c, const d2pc_sectors_fov *fovs, int n_fovs, uint8_t *covered) {
  const double two_pi = 6.283185307179586476925286766559;
  const bool elevation = c.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION;
  const double lo = double(c.u_min), span = double(c.u_max) - double(c.u_min);
  for (int layer = 0; layer < c.n_layers; ++layer) {
    double el = 0.0;
    if (elevation) {
      const double e0 = lo + (double(layer) * span) / double(c.n_layers), e1 = lo + (double(layer + 1) * span) / double(c.n_layers);
      el = (e0 + e1) / 2.0;
    }
    for (int k = 0; k < c.n_sectors; ++k) {
      const double az = c.azimuth0 + two_pi * (double(k) + 0.5) / double(c.n_sectors);
      bool in = false;
      for (int v = 0; v < n_fovs && !in; ++v) {
        const d2pc_sectors_fov &f = fovs[v];
        in = std::fabs(std::remainder(az - f.yaw, two_pi)) <= f.h_fov / 2.0 - f.margin;
        if (elevation) in = in && std::fabs(el - f.pitch) <= f.v_fov / 2.0 - f.margin;
      }
      covered[size_t(layer) * size_t(c.n_sectors) + size_t(k)] = in ? 1 : 0;
    }
  }
}

// One update as d2pc_sectors_memory.hip's kernel gets it (d2pc_sectors_memory_capi.hip fills it).
struct MemoryLaunch {
  MemoryPlan plan;
  const void *points;
  const uint32_t *count, *nearest;
  const void *step;            // DEVICE: d2pc_sectors_memory_step
  const uint8_t *covered;
  const float *table;          // DEVICE: half x (c, s), then plan.grid.elev x (ce, se)
  void *buffers;               // DEVICE: 2 x n_cells records; the launch reads buffer *parity and writes the other
  uint32_t *parity;            // DEVICE: 0 or 1, flipped by the launch's last store
  float *range;
  uint16_t *distance_cm;
  uint32_t *age;
  void *records;
  uint32_t bound, step16;      // the position bound; 16-byte units of a record of `points`
  void *stream;
};
// hipError_t as int
int launch_memory_update(const MemoryLaunch &a);
int launch_memory_reset(void *buffers, int n_cells, void *stream);

}  // namespace sectors
}  // namespace d2pc
