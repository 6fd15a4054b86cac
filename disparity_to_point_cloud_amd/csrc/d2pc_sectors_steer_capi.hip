// d2pc_sectors_steer_capi.hip -- include/d2pc_sectors.h: the steer session (the two reach tables in device memory) and
// its one asynchronous call.  Everything that needs no device -- the refusals, the tables' values, the cell of a goal
// direction -- is d2pc_sectors_steer_plan.hpp's; this file adds the device.
#include <new>
#include <vector>

#include "d2pc_sectors_session.hpp"
#include "d2pc_sectors_steer_plan.hpp"

using namespace d2pc::sectors;

struct d2pc_sectors_steer {
  SteerPlan plan{};
  int device = 0;
  uint16_t *d_reach = nullptr;   // reach_s (n_layers x (Wa + 1)), then reach_l (We + 1)
  char err[256] = "";
};

extern "C" {

void d2pc_sectors_steer_config_init(d2pc_sectors_steer_config *scfg) {
  if (!scfg) return;
  memset(scfg, 0, sizeof *scfg);
  scfg->struct_size = sizeof *scfg;
  scfg->radius = 0.5f;
  scfg->max_reach_sectors = 8, scfg->max_reach_layers = 0;
  scfg->free_cm = 65535u, scfg->min_clearance_cm = 100u, scfg->horizon_cm = 1000u;
  scfg->w_goal = 16u, scfg->w_prev = 4u, scfg->w_near = 1u;
}

int d2pc_sectors_steer_reach(const d2pc_sectors_config *grid, const d2pc_sectors_steer_config *scfg, uint16_t *reach_sectors,
                             int sectors_capacity, uint16_t *reach_layers, int layers_capacity) {
  if (!reach_sectors || !reach_layers) return -D2PC_ERR_INVALID_ARG;
  SteerPlan p;
  const int st = make_steer_plan(grid, scfg, &p);
  if (st != D2PC_OK) return -st;
  if (sectors_capacity < p.reach_s_entries || layers_capacity < p.reach_l_entries) return -D2PC_ERR_CAPACITY;
  fill_reach(*grid, *scfg, reach_sectors, reach_layers);
  return p.reach_s_entries;
}

int d2pc_sectors_steer_goal_cell(const d2pc_sectors_config *grid, double yaw, double pitch_or_layer, uint32_t *sector, uint32_t *layer) {
  if (!sector || !layer) return D2PC_ERR_INVALID_ARG;
  Plan p;
  const int st = make_plan(grid, &p);
  return st != D2PC_OK ? st : steer_goal_cell(*grid, yaw, pitch_or_layer, sector, layer);
}

int d2pc_sectors_steer_create(const d2pc_sectors_config *grid, const d2pc_sectors_steer_config *scfg, d2pc_sectors_steer **out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  SteerPlan p;
  const int st = make_steer_plan(grid, scfg, &p);
  if (st != D2PC_OK) return st;
  if (!device_exists(grid->device_id)) return D2PC_ERR_NO_DEVICE;
  DeviceGuard guard(grid->device_id);
  if (!guard.ok) return D2PC_ERR_NO_DEVICE;
  d2pc_sectors_steer *s = new (std::nothrow) d2pc_sectors_steer();
  if (!s) return D2PC_ERR_OUT_OF_MEMORY;
  s->plan = p, s->device = grid->device_id;
  std::vector<uint16_t> reach(size_t(p.reach_s_entries) + size_t(p.reach_l_entries));
  fill_reach(*grid, *scfg, reach.data(), reach.data() + p.reach_s_entries);
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&s->d_reach), reach.size() * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMemcpy(s->d_reach, reach.data(), reach.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)d2pc_sectors_steer_destroy(s);
    return e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE;
  }
  *out = s;
  return D2PC_OK;
}

int d2pc_sectors_steer_destroy(d2pc_sectors_steer *s) {
  if (!s) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(s->device);
  if (s->d_reach) (void)hipFree(s->d_reach);   // (hipFree waits for the device's work)
  delete s;
  return D2PC_OK;
}

const char *d2pc_sectors_steer_last_error(const d2pc_sectors_steer *s) { return s ? s->err : "null session"; }

void d2pc_sectors_steer_desc_init(d2pc_sectors_steer_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->n_candidates = 1;
}

int d2pc_sectors_steer_desc_check(const d2pc_sectors_config *grid, const d2pc_sectors_steer_config *scfg,
                                  const d2pc_sectors_steer_desc *desc) {
  SteerPlan p;
  const int st = make_steer_plan(grid, scfg, &p);
  return st != D2PC_OK ? st : check_steer_desc(p, desc);
}

int d2pc_sectors_steer_device(d2pc_sectors_steer *s, const d2pc_sectors_steer_desc *d, void *stream) {
  if (!s) return D2PC_ERR_INVALID_ARG;
  const int st = check_steer_desc(s->plan, d, s->err, sizeof s->err);
  if (st != D2PC_OK) return st;
  DeviceGuard guard(s->device);
  if (!guard.ok) return fail(s->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", s->device);
  SteerLaunch a;
  a.plan = s->plan;
  a.distance_cm = d->distance_cm, a.allowed = d->allowed, a.step = d->step, a.reach = s->d_reach;
  a.clearance_cm = d->clearance_cm, a.cost = d->cost, a.candidates = d->candidates, a.summary = d->summary;
  a.n_candidates = d->candidates ? d->n_candidates : 0;
  a.stream = stream;   // NULL = HIP's default stream
  const hipError_t e = hipError_t(launch_steer(a));
  if (e != hipSuccess) return fail(s->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

}  // extern "C"
