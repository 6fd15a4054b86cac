// d2pc_sectors_slope_capi.hip -- include/d2pc_sectors.h: the slope session (the reducing blocks' slabs and the 14 bytes per
// cell that the merge hands to the sites, in device memory) and its one asynchronous call.  Everything that needs no device --
// the refusals, scale and max_tilt2, the sizes -- is d2pc_sectors_slope_plan.hpp's; this file adds the device.
#include <new>

#include "d2pc_sectors_session.hpp"
#include "d2pc_sectors_slope_plan.hpp"

using namespace d2pc::sectors;

struct d2pc_sectors_slope {
  SlopePlan plan{};
  int device = 0, blocks = 0;
  void *d_slabs = nullptr;     // blocks x plan.block_bytes
  void *d_hand_on = nullptr;   // count, level_q, resid_q2 (4 bytes x n_cells each), then flat and fitted (n_cells each)
  char err[256] = "";
};

extern "C" {

void d2pc_sectors_slope_config_init(d2pc_sectors_slope_config *scfg) {
  if (!scfg) return;
  memset(scfg, 0, sizeof *scfg);
  scfg->struct_size = sizeof *scfg;
  scfg->sub = 8;
  scfg->max_slope = 0.26794919f;   // tanf of 15 degrees
}

int d2pc_sectors_slope_geometry(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                d2pc_sectors_slope_geometry_t *out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  SlopePlan p;
  const int st = make_slope_plan(gcfg, scfg, &p);
  if (st != D2PC_OK) return st;
  fill_slope_geometry(p, out);
  return D2PC_OK;
}

float d2pc_sectors_slope_of_degrees(double degrees) { return slope_of_degrees(degrees); }

int d2pc_sectors_slope_create(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg, d2pc_sectors_slope **out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  SlopePlan p;
  const int st = make_slope_plan(gcfg, scfg, &p);
  if (st != D2PC_OK) return st;
  if (!device_exists(gcfg->device_id)) return D2PC_ERR_NO_DEVICE;
  DeviceGuard guard(gcfg->device_id);
  if (!guard.ok) return D2PC_ERR_NO_DEVICE;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, gcfg->device_id) != hipSuccess || cus < 1) return D2PC_ERR_DEVICE;
  d2pc_sectors_slope *s = new (std::nothrow) d2pc_sectors_slope();
  if (!s) return D2PC_ERR_OUT_OF_MEMORY;
  s->plan = p, s->device = gcfg->device_id;
  s->blocks = ground_blocks(p.ground.max_points, p.blocks_per_cu, cus);
  hipError_t e = hipMalloc(&s->d_slabs, size_t(s->blocks) * p.block_bytes);
  if (e == hipSuccess) e = hipMalloc(&s->d_hand_on, kSlopeHandOnBytes * size_t(p.ground.n_cells));
  if (e == hipSuccess) e = hipError_t(prepare_slope_kernels(p));
  if (e != hipSuccess) {
    (void)d2pc_sectors_slope_destroy(s);
    return e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE;
  }
  *out = s;
  return D2PC_OK;
}

int d2pc_sectors_slope_destroy(d2pc_sectors_slope *s) {
  if (!s) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(s->device);
  if (s->d_slabs) (void)hipFree(s->d_slabs);   // (hipFree waits for the device's work)
  if (s->d_hand_on) (void)hipFree(s->d_hand_on);
  delete s;
  return D2PC_OK;
}

const char *d2pc_sectors_slope_last_error(const d2pc_sectors_slope *s) { return s ? s->err : "null session"; }

int d2pc_sectors_slope_blocks(const d2pc_sectors_slope *s) { return s ? s->blocks : 0; }

void d2pc_sectors_slope_desc_init(d2pc_sectors_slope_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->point_step = 16;
  desc->n_clouds = 1, desc->n_candidates = 1;
}

int d2pc_sectors_slope_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_slope_config *scfg,
                                  const d2pc_sectors_slope_desc *desc) {
  SlopePlan p;
  const int st = make_slope_plan(gcfg, scfg, &p);
  return st != D2PC_OK ? st : check_slope_desc(p, desc);
}

int d2pc_sectors_slope_process_device(d2pc_sectors_slope *s, const d2pc_sectors_slope_desc *d, void *stream) {
  if (!s) return D2PC_ERR_INVALID_ARG;
  const int st = check_slope_desc(s->plan, d, s->err, sizeof s->err);
  if (st != D2PC_OK) return st;
  DeviceGuard guard(s->device);
  if (!guard.ok) return fail(s->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", s->device);
  SlopeLaunch a;
  a.plan = s->plan;
  a.walk = cloud_walk(*d), a.step = d->step, a.allowed = d->allowed;
  a.slabs = s->d_slabs, a.hand_on = s->d_hand_on;
  a.count = d->count, a.sum = d->sum, a.sum2 = d->sum2, a.moments = d->moments;
  a.slope_a = d->slope_a, a.slope_b = d->slope_b, a.level_q = d->level_q, a.resid_q2 = d->resid_q2, a.flat = d->flat;
  a.site = d->site, a.candidates = d->candidates, a.summary = d->summary;
  a.n_candidates = d->candidates ? d->n_candidates : 0;
  a.blocks = a.walk.shares < uint64_t(s->blocks) ? int(a.walk.shares) : s->blocks;   // (a block without a share would store an empty slab)
  a.stream = stream;   // NULL = HIP's default stream
  const hipError_t e = hipError_t(launch_slope(a));
  if (e != hipSuccess) return fail(s->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

}  // extern "C"
