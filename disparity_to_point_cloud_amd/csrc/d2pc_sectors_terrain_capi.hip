// d2pc_sectors_terrain_capi.hip -- include/d2pc_sectors.h: the terrain session (one state block in device memory: 16 headers
// and `depth` stored tables) and its one asynchronous update.  Everything that needs no device -- the refusals and the
// sizes -- is d2pc_sectors_terrain_plan.hpp's; this file adds the device.
#include <new>

#include "d2pc_sectors_session.hpp"
#include "d2pc_sectors_terrain_plan.hpp"

using namespace d2pc::sectors;

struct d2pc_sectors_terrain {
  TerrainPlan plan{};
  int device = 0;
  void *d_state = nullptr;   // plan.state_bytes: the headers, then the tables
  char err[256] = "";
};

extern "C" {

void d2pc_sectors_terrain_config_init(d2pc_sectors_terrain_config *tcfg) {
  if (!tcfg) return;
  memset(tcfg, 0, sizeof *tcfg);
  tcfg->struct_size = sizeof *tcfg;
  tcfg->depth = 8;
}

int d2pc_sectors_terrain_geometry(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_terrain_config *tcfg,
                                  d2pc_sectors_terrain_geometry_t *out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  TerrainPlan p;
  const int st = make_terrain_plan(gcfg, tcfg, &p);
  if (st != D2PC_OK) return st;
  fill_terrain_geometry(p, out);
  return D2PC_OK;
}

int d2pc_sectors_terrain_create(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_terrain_config *tcfg, d2pc_sectors_terrain **out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  TerrainPlan p;
  const int st = make_terrain_plan(gcfg, tcfg, &p);
  if (st != D2PC_OK) return st;
  if (!device_exists(gcfg->device_id)) return D2PC_ERR_NO_DEVICE;
  DeviceGuard guard(gcfg->device_id);
  if (!guard.ok) return D2PC_ERR_NO_DEVICE;
  d2pc_sectors_terrain *t = new (std::nothrow) d2pc_sectors_terrain();
  if (!t) return D2PC_ERR_OUT_OF_MEMORY;
  t->plan = p, t->device = gcfg->device_id;
  hipError_t e = hipMalloc(&t->d_state, p.state_bytes);
  if (e == hipSuccess) e = hipMemset(t->d_state, 0, p.state_bytes);   // (once, at creation: the updates use no memset)
  if (e != hipSuccess) {
    (void)d2pc_sectors_terrain_destroy(t);
    return e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE;
  }
  *out = t;
  return D2PC_OK;
}

int d2pc_sectors_terrain_destroy(d2pc_sectors_terrain *t) {
  if (!t) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(t->device);
  if (t->d_state) (void)hipFree(t->d_state);   // (hipFree waits for the device's work)
  delete t;
  return D2PC_OK;
}

const char *d2pc_sectors_terrain_last_error(const d2pc_sectors_terrain *t) { return t ? t->err : "null session"; }

int d2pc_sectors_terrain_state(const d2pc_sectors_terrain *t, void **device_ptr, size_t *bytes) {
  if (!t) return D2PC_ERR_INVALID_ARG;
  if (device_ptr) *device_ptr = t->d_state;
  if (bytes) *bytes = t->plan.state_bytes;
  return D2PC_OK;
}

int d2pc_sectors_terrain_reset_device(d2pc_sectors_terrain *t, void *stream) {
  if (!t) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(t->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", t->device);
  const hipError_t e = hipError_t(launch_terrain_reset(t->d_state, stream));
  if (e != hipSuccess) return fail(t->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

void d2pc_sectors_terrain_desc_init(d2pc_sectors_terrain_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->n_candidates = 1;
}

int d2pc_sectors_terrain_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_terrain_config *tcfg,
                                    const d2pc_sectors_terrain_desc *desc) {
  TerrainPlan p;
  const int st = make_terrain_plan(gcfg, tcfg, &p);
  return st != D2PC_OK ? st : check_terrain_desc(p, desc);
}

int d2pc_sectors_terrain_update_device(d2pc_sectors_terrain *t, const d2pc_sectors_terrain_desc *d, void *stream) {
  if (!t) return D2PC_ERR_INVALID_ARG;
  int st = check_terrain_desc(t->plan, d, t->err, sizeof t->err);
  if (st == D2PC_OK) st = check_terrain_state(t->plan, d, t->d_state, t->err, sizeof t->err);
  if (st != D2PC_OK) return st;
  DeviceGuard guard(t->device);
  if (!guard.ok) return fail(t->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", t->device);
  TerrainLaunch a;
  a.plan = t->plan;
  a.state = t->d_state;
  a.step = d->step, a.frame_count = d->frame_count, a.frame_sum = d->frame_sum, a.frame_sum2 = d->frame_sum2, a.allowed = d->allowed;
  a.count = d->count, a.sum = d->sum, a.sum2 = d->sum2, a.mean_q = d->mean_q, a.spread_q2 = d->spread_q2, a.flat = d->flat;
  a.site = d->site, a.candidates = d->candidates, a.summary = d->summary, a.status = d->status;
  a.n_candidates = d->candidates ? d->n_candidates : 0;
  a.stream = stream;   // NULL = HIP's default stream
  const hipError_t e = hipError_t(launch_terrain(a));
  if (e != hipSuccess) return fail(t->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

}  // extern "C"
