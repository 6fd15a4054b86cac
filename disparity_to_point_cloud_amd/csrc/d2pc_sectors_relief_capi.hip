// d2pc_sectors_relief_capi.hip -- include/d2pc_sectors.h: the relief session (one state block in device memory: 16 headers
// and `depth` stored tables of the slope's ten sums; and the 14 bytes per cell that the window launch hands to the sites) and
// its one asynchronous update.  Everything that needs no device -- the refusals and the sizes -- is
// d2pc_sectors_relief_plan.hpp's; this file adds the device.
#include <new>

#include "d2pc_sectors_relief_plan.hpp"
#include "d2pc_sectors_session.hpp"

using namespace d2pc::sectors;

struct d2pc_sectors_relief {
  ReliefPlan plan{};
  int device = 0;
  void *d_state = nullptr;     // plan.state_bytes: the headers, then the tables
  void *d_hand_on = nullptr;   // count, level_q, resid_q2 (4 bytes x n_cells each), then flat and fitted (n_cells each)
  char err[256] = "";
};

extern "C" {

int d2pc_sectors_relief_geometry(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                 const d2pc_sectors_terrain_config *tcfg, d2pc_sectors_relief_geometry_t *out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  ReliefPlan p;
  const int st = make_relief_plan(gcfg, scfg, tcfg, &p);
  if (st != D2PC_OK) return st;
  fill_relief_geometry(p, out);
  return D2PC_OK;
}

int d2pc_sectors_relief_create(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                               const d2pc_sectors_terrain_config *tcfg, d2pc_sectors_relief **out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  ReliefPlan p;
  const int st = make_relief_plan(gcfg, scfg, tcfg, &p);
  if (st != D2PC_OK) return st;
  if (!device_exists(gcfg->device_id)) return D2PC_ERR_NO_DEVICE;
  DeviceGuard guard(gcfg->device_id);
  if (!guard.ok) return D2PC_ERR_NO_DEVICE;
  d2pc_sectors_relief *r = new (std::nothrow) d2pc_sectors_relief();
  if (!r) return D2PC_ERR_OUT_OF_MEMORY;
  r->plan = p, r->device = gcfg->device_id;
  hipError_t e = hipMalloc(&r->d_state, p.state_bytes);
  if (e == hipSuccess) e = hipMemset(r->d_state, 0, p.state_bytes);   // (once, at creation: the updates use no memset)
  if (e == hipSuccess) e = hipMalloc(&r->d_hand_on, kSlopeHandOnBytes * size_t(p.slope.ground.n_cells));
  if (e != hipSuccess) {
    (void)d2pc_sectors_relief_destroy(r);
    return e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE;
  }
  *out = r;
  return D2PC_OK;
}

int d2pc_sectors_relief_destroy(d2pc_sectors_relief *r) {
  if (!r) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(r->device);
  if (r->d_state) (void)hipFree(r->d_state);   // (hipFree waits for the device's work)
  if (r->d_hand_on) (void)hipFree(r->d_hand_on);
  delete r;
  return D2PC_OK;
}

const char *d2pc_sectors_relief_last_error(const d2pc_sectors_relief *r) { return r ? r->err : "null session"; }

int d2pc_sectors_relief_state(const d2pc_sectors_relief *r, void **device_ptr, size_t *bytes) {
  if (!r) return D2PC_ERR_INVALID_ARG;
  if (device_ptr) *device_ptr = r->d_state;
  if (bytes) *bytes = r->plan.state_bytes;
  return D2PC_OK;
}

int d2pc_sectors_relief_reset_device(d2pc_sectors_relief *r, void *stream) {
  if (!r) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(r->device);
  if (!guard.ok) return fail(r->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", r->device);
  const hipError_t e = hipError_t(launch_relief_reset(r->d_state, stream));
  if (e != hipSuccess) return fail(r->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

void d2pc_sectors_relief_desc_init(d2pc_sectors_relief_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->n_candidates = 1;
}

int d2pc_sectors_relief_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                   const d2pc_sectors_terrain_config *tcfg, const d2pc_sectors_relief_desc *desc) {
  ReliefPlan p;
  const int st = make_relief_plan(gcfg, scfg, tcfg, &p);
  return st != D2PC_OK ? st : check_relief_desc(p, desc);
}

int d2pc_sectors_relief_update_device(d2pc_sectors_relief *r, const d2pc_sectors_relief_desc *d, void *stream) {
  if (!r) return D2PC_ERR_INVALID_ARG;
  int st = check_relief_desc(r->plan, d, r->err, sizeof r->err);
  if (st == D2PC_OK) st = check_relief_state(r->plan, d, r->d_state, r->err, sizeof r->err);
  if (st != D2PC_OK) return st;
  DeviceGuard guard(r->device);
  if (!guard.ok) return fail(r->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", r->device);
  ReliefLaunch a;
  a.plan = r->plan;
  a.state = r->d_state, a.hand_on = r->d_hand_on;
  a.desc = d;
  a.stream = stream;   // NULL = HIP's default stream
  const hipError_t e = hipError_t(launch_relief(a));
  if (e != hipSuccess) return fail(r->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

}  // extern "C"
