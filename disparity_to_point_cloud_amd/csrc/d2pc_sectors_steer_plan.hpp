// d2pc_sectors_steer_plan.hpp -- the host side of the steer session of include/d2pc_sectors.h that needs no device: what a
// steer configuration and a steer descriptor are refused for, the reach tables (in double, rounded down once), the cell
// of a goal direction and the LDS of the one block.  The grid's own refusals are d2pc_sectors_plan.hpp's (make_plan).
// Host code only and no HIP: plain g++ compiles it (tests/test_sectors_steer_cpu.py, tests/cpp/sectors_steer_plan_main.cpp).
#pragma once
#include "d2pc_sectors_plan.hpp"

namespace d2pc {
namespace sectors {

constexpr int kSteerThreads = 1024;      // the one block of a steer call
constexpr int kSteerWaves = kSteerThreads / 64;
constexpr int kSteerPerLane = (kMaxCells + kSteerThreads - 1) / kSteerThreads;   // cells a lane holds: 6
constexpr uint32_t kSteerNothing = 65535u;    // a d or a clearance with nothing there
constexpr uint32_t kSteerFarthest = 65534u;   // the largest reach of a neighbour
static_assert(kSteerPerLane * kSteerThreads >= kMaxCells, "a lane's cells cover the largest grid");

struct SteerPlan {
  Plan grid;
  int wa, we;                // max_reach_sectors, max_reach_layers
  uint32_t free_cm, min_clearance_cm, horizon_cm, w_goal, w_prev, w_near;
  int reach_s_entries;       // n_layers x (wa + 1)
  int reach_l_entries;       // we + 1
  size_t lds_bytes;          // two planes of 16-bit cells, then the two tables
};

// D2PC_OK and *p filled, or the refusal: the grid's, as make_plan makes them, then the steer configuration's
inline int make_steer_plan(const d2pc_sectors_config *grid, const d2pc_sectors_steer_config *s, SteerPlan *p, char *msg = nullptr,
                           size_t msg_len = 0) {
  const int st = make_plan(grid, &p->grid, msg, msg_len);
  if (st != D2PC_OK) return st;
  if (!s || s->struct_size != sizeof(d2pc_sectors_steer_config)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_steer_config");
  if (!std::isfinite(s->radius) || !(s->radius > 0.0f)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "the radius must be finite and > 0");
  if (s->w_goal > D2PC_SECTORS_STEER_MAX_WEIGHT || s->w_prev > D2PC_SECTORS_STEER_MAX_WEIGHT || s->w_near > D2PC_SECTORS_STEER_MAX_WEIGHT)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "weights of %u / %u / %u: %d at the most", s->w_goal, s->w_prev, s->w_near, D2PC_SECTORS_STEER_MAX_WEIGHT);
  if (s->free_cm > 65535u || s->min_clearance_cm > 65535u || s->horizon_cm > 65535u)
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "free_cm, min_clearance_cm or horizon_cm does not fit 16 bits");
  if (s->max_reach_sectors < 0 || s->max_reach_sectors > D2PC_SECTORS_STEER_MAX_REACH_SECTORS)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "max_reach_sectors of %d: 0 .. %d", s->max_reach_sectors, D2PC_SECTORS_STEER_MAX_REACH_SECTORS);
  if (s->max_reach_layers < 0 || s->max_reach_layers > D2PC_SECTORS_STEER_MAX_REACH_LAYERS)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "max_reach_layers of %d: 0 .. %d", s->max_reach_layers, D2PC_SECTORS_STEER_MAX_REACH_LAYERS);
  if (s->max_reach_sectors > p->grid.half)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "max_reach_sectors of %d: half of the %d sectors at the most", s->max_reach_sectors, p->grid.n_sectors);
  if (s->max_reach_layers > p->grid.n_layers - 1)
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "max_reach_layers of %d with %d layers", s->max_reach_layers, p->grid.n_layers);
  if (s->max_reach_layers > 0 && p->grid.layer_kind == D2PC_SECTORS_LAYERS_HEIGHT && !(std::isfinite(grid->u_min) && std::isfinite(grid->u_max)))
    D2PC_SECTORS_REFUSE(D2PC_ERR_BAD_SIZE, "a reach over layers needs a finite height band");
  p->wa = s->max_reach_sectors, p->we = s->max_reach_layers;
  p->free_cm = s->free_cm, p->min_clearance_cm = s->min_clearance_cm, p->horizon_cm = s->horizon_cm;
  p->w_goal = s->w_goal, p->w_prev = s->w_prev, p->w_near = s->w_near;
  p->reach_s_entries = p->grid.n_layers * (p->wa + 1), p->reach_l_entries = p->we + 1;
  p->lds_bytes = 2u * 2u * size_t(p->grid.n_cells) + 2u * size_t(p->reach_s_entries + p->reach_l_entries);
  p->lds_bytes = (p->lds_bytes + 15u) & ~size_t(15);
  return D2PC_OK;
}

// reach(theta) of the specification
inline uint16_t steer_reach(double rho, double theta) {
  const double half_pi = 1.57079632679489661923132169163975;
  if (!(theta > 0.0)) return uint16_t(kSteerFarthest);
  const double q = theta < half_pi ? std::floor(100.0 * rho / std::sin(theta)) : std::floor(100.0 * rho);
  return q >= double(kSteerFarthest) ? uint16_t(kSteerFarthest) : uint16_t(q);   // (q >= 0: rho > 0 and sin(theta) > 0)
}

// reach_s: n_layers rows of wa + 1; reach_l: we + 1 (d2pc_sectors.h).  `c` and `s` passed make_steer_plan
inline void fill_reach(const d2pc_sectors_config &c, const d2pc_sectors_steer_config &s, uint16_t *reach_s, uint16_t *reach_l) {
  const double two_pi = 6.283185307179586476925286766559;
  const bool elevation = c.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION;
  const double rho = double(s.radius), alpha = two_pi / double(c.n_sectors);
  const int wa = s.max_reach_sectors, we = s.max_reach_layers;
  const double lo = double(c.u_min), span = double(c.u_max) - double(c.u_min);
  const double eps = span / double(c.n_layers);   // (not finite without a height band: then we is 0 and cos_i is 1)
  for (int i = 0; i < c.n_layers; ++i) {
    const double cos_i = elevation ? std::cos(lo + (double(i) * span) / double(c.n_layers) + eps / 2.0) : 1.0;
    uint16_t *row = reach_s + size_t(i) * size_t(wa + 1);
    row[0] = uint16_t(kSteerNothing);
    for (int k = 1; k <= wa; ++k) row[k] = steer_reach(rho, (double(k) - 0.5) * alpha * cos_i);
  }
  reach_l[0] = uint16_t(kSteerNothing);
  for (int k = 1; k <= we; ++k) {
    const double off = (double(k) - 0.5) * eps;
    reach_l[k] = elevation ? steer_reach(rho, off) : uint16_t(off < rho ? kSteerFarthest : 0u);
  }
}

// the cell of a direction (d2pc_sectors.h); `c` passed make_plan
inline int steer_goal_cell(const d2pc_sectors_config &c, double yaw, double pitch_or_layer, uint32_t *sector, uint32_t *layer,
                           char *msg = nullptr, size_t msg_len = 0) {
  const double two_pi = 6.283185307179586476925286766559;
  if (!std::isfinite(yaw) || !std::isfinite(pitch_or_layer)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "the direction is not finite");
  double x = std::fmod(yaw - c.azimuth0, two_pi);
  if (x < 0.0) x += two_pi;
  int k = int(std::floor(x / (two_pi / double(c.n_sectors))));
  if (k > c.n_sectors - 1) k = c.n_sectors - 1;   // (x + 2 pi may round to a whole turn)
  int i = 0;
  if (c.layer_kind == D2PC_SECTORS_LAYERS_ELEVATION) {
    const double lo = double(c.u_min), span = double(c.u_max) - double(c.u_min);
    if (!(pitch_or_layer >= lo) || !(pitch_or_layer < lo + (double(c.n_layers) * span) / double(c.n_layers)))
      D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a pitch of %g lies outside the elevation band", pitch_or_layer);
    for (int j = 1; j < c.n_layers; ++j) i += pitch_or_layer >= lo + (double(j) * span) / double(c.n_layers) ? 1 : 0;
  } else {
    if (!(pitch_or_layer >= 0.0) || !(pitch_or_layer < double(c.n_layers)))
      D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "a layer of %g with %d layers", pitch_or_layer, c.n_layers);
    i = int(std::floor(pitch_or_layer));
  }
  *sector = uint32_t(k), *layer = uint32_t(i);
  return D2PC_OK;
}

// what d2pc_sectors_steer_device refuses of a descriptor, for a session of plan `p`
inline int check_steer_desc(const SteerPlan &p, const d2pc_sectors_steer_desc *d, char *msg = nullptr, size_t msg_len = 0) {
  if (!d || d->struct_size != sizeof(d2pc_sectors_steer_desc)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "bad d2pc_sectors_steer_desc");
  if (!d->distance_cm) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "distance_cm is null");
  if (!d->step) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "step is null");
  if (!d->clearance_cm && !d->cost && !d->candidates && !d->summary) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "no output is given");
  if (d->candidates && (d->n_candidates < 1 || d->n_candidates > D2PC_SECTORS_STEER_MAX_CANDIDATES))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "n_candidates of %d: 1 .. %d", d->n_candidates, D2PC_SECTORS_STEER_MAX_CANDIDATES);
  if (misaligned(d->distance_cm, 2) || misaligned(d->step, 4) || misaligned(d->clearance_cm, 2) || misaligned(d->cost, 4) ||
      misaligned(d->summary, 4))
    D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "distance_cm, step or an output is not aligned to its type");
  if (misaligned(d->candidates, 8)) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "candidates must be 8-byte aligned");
  const size_t n = size_t(p.grid.n_cells);
  const void *ins[3] = {d->distance_cm, d->allowed, d->step};
  const size_t in_bytes[3] = {n * 2u, n, sizeof(d2pc_sectors_steer_step)};
  const void *outs[4] = {d->clearance_cm, d->cost, d->candidates, d->summary};
  const size_t out_bytes[4] = {n * 2u, n * 4u, d->candidates ? size_t(d->n_candidates) * 8u : 0u, 16u};
  for (int i = 0; i < 4; ++i) {
    for (int k = 0; k < 3; ++k)
      if (hulls_meet(outs[i], out_bytes[i], ins[k], in_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "an output overlaps an input");
    for (int k = i + 1; k < 4; ++k)
      if (hulls_meet(outs[i], out_bytes[i], outs[k], out_bytes[k])) D2PC_SECTORS_REFUSE(D2PC_ERR_INVALID_ARG, "two outputs overlap");
  }
  return D2PC_OK;
}

// One call as d2pc_sectors_steer.hip's kernel gets it (d2pc_sectors_steer_capi.hip fills it).
struct SteerLaunch {
  SteerPlan plan;
  const uint16_t *distance_cm;
  const uint8_t *allowed;
  const void *step;            // DEVICE: d2pc_sectors_steer_step
  const uint16_t *reach;       // DEVICE: reach_s (plan.reach_s_entries), then reach_l (plan.reach_l_entries)
  uint16_t *clearance_cm;
  uint32_t *cost;
  void *candidates;
  uint32_t *summary;
  int n_candidates;            // 0 without candidates
  void *stream;
};
// hipError_t as int
int launch_steer(const SteerLaunch &a);

}  // namespace sectors
}  // namespace d2pc
