// d2pc_sectors_ground_capi.hip -- include/d2pc_sectors.h: the ground session (the reducing blocks' slabs and the 13 bytes per
// cell that the merge hands to the sites, in device memory) and its one asynchronous call.  Everything that needs no device --
// the refusals, inv_c / inv_q, the number of blocks -- is d2pc_sectors_ground_plan.hpp's; this file adds the device.
#include <new>

#include "d2pc_sectors_session.hpp"
#include "d2pc_sectors_ground_plan.hpp"

using namespace d2pc::sectors;

struct d2pc_sectors_ground {
  GroundPlan plan{};
  int device = 0, blocks = 0;
  void *d_slabs = nullptr;     // blocks x plan.block_bytes
  void *d_hand_on = nullptr;   // count, mean_q, spread_q2 (4 bytes x n_cells each), then flat (n_cells)
  char err[256] = "";
};

extern "C" {

void d2pc_sectors_ground_config_init(d2pc_sectors_ground_config *gcfg) {
  if (!gcfg) return;
  memset(gcfg, 0, sizeof *gcfg);
  gcfg->struct_size = sizeof *gcfg;
  gcfg->n_a = 16, gcfg->n_b = 16;
  gcfg->cell_size = 0.5f, gcfg->quantum = 0.002f;
  gcfg->axes[0] = 1, gcfg->axes[1] = 2, gcfg->axes[2] = 3;
  gcfg->min_count = 4u, gcfg->max_spread_q2 = 625u, gcfg->max_step_q = 50u;
  gcfg->window = 1;
  gcfg->w_dist = 1u, gcfg->w_rough = 1u, gcfg->rough_cap = 65535u;
}

int d2pc_sectors_ground_geometry(const d2pc_sectors_ground_config *gcfg, d2pc_sectors_ground_geometry_t *out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  GroundPlan p;
  const int st = make_ground_plan(gcfg, &p);
  if (st != D2PC_OK) return st;
  fill_ground_geometry(p, out);
  return D2PC_OK;
}

uint32_t d2pc_sectors_ground_spread_of_std(double quantum, double std_dev) { return ground_spread_of_std(quantum, std_dev); }

int d2pc_sectors_ground_create(const d2pc_sectors_ground_config *gcfg, d2pc_sectors_ground **out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  GroundPlan p;
  const int st = make_ground_plan(gcfg, &p);
  if (st != D2PC_OK) return st;
  if (!device_exists(gcfg->device_id)) return D2PC_ERR_NO_DEVICE;
  DeviceGuard guard(gcfg->device_id);
  if (!guard.ok) return D2PC_ERR_NO_DEVICE;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, gcfg->device_id) != hipSuccess || cus < 1) return D2PC_ERR_DEVICE;
  d2pc_sectors_ground *g = new (std::nothrow) d2pc_sectors_ground();
  if (!g) return D2PC_ERR_OUT_OF_MEMORY;
  g->plan = p, g->device = gcfg->device_id;
  g->blocks = ground_blocks(p.max_points, p.blocks_per_cu, cus);
  hipError_t e = hipMalloc(&g->d_slabs, size_t(g->blocks) * p.block_bytes);
  if (e == hipSuccess) e = hipMalloc(&g->d_hand_on, kGroundHandOnBytes * size_t(p.n_cells));
  if (e == hipSuccess) e = hipError_t(prepare_ground_kernels(p));
  if (e != hipSuccess) {
    (void)d2pc_sectors_ground_destroy(g);
    return e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE;
  }
  *out = g;
  return D2PC_OK;
}

int d2pc_sectors_ground_destroy(d2pc_sectors_ground *g) {
  if (!g) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(g->device);
  if (g->d_slabs) (void)hipFree(g->d_slabs);   // (hipFree waits for the device's work)
  if (g->d_hand_on) (void)hipFree(g->d_hand_on);
  delete g;
  return D2PC_OK;
}

const char *d2pc_sectors_ground_last_error(const d2pc_sectors_ground *g) { return g ? g->err : "null session"; }

int d2pc_sectors_ground_blocks(const d2pc_sectors_ground *g) { return g ? g->blocks : 0; }

void d2pc_sectors_ground_desc_init(d2pc_sectors_ground_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->point_step = 16;
  desc->n_clouds = 1, desc->n_candidates = 1;
}

int d2pc_sectors_ground_desc_check(const d2pc_sectors_ground_config *gcfg, const d2pc_sectors_ground_desc *desc) {
  GroundPlan p;
  const int st = make_ground_plan(gcfg, &p);
  return st != D2PC_OK ? st : check_ground_desc(p, desc);
}

int d2pc_sectors_ground_process_device(d2pc_sectors_ground *g, const d2pc_sectors_ground_desc *d, void *stream) {
  if (!g) return D2PC_ERR_INVALID_ARG;
  const int st = check_ground_desc(g->plan, d, g->err, sizeof g->err);
  if (st != D2PC_OK) return st;
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(g->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", g->device);
  GroundLaunch a;
  a.plan = g->plan;
  a.walk = cloud_walk(*d), a.step = d->step, a.allowed = d->allowed;
  a.slabs = g->d_slabs, a.hand_on = g->d_hand_on;
  a.count = d->count, a.sum = d->sum, a.sum2 = d->sum2, a.mean_q = d->mean_q, a.spread_q2 = d->spread_q2, a.flat = d->flat;
  a.site = d->site, a.candidates = d->candidates, a.summary = d->summary;
  a.n_candidates = d->candidates ? d->n_candidates : 0;
  a.blocks = a.walk.shares < uint64_t(g->blocks) ? int(a.walk.shares) : g->blocks;   // (a block without a share would store an empty slab)
  a.stream = stream;   // NULL = HIP's default stream
  const hipError_t e = hipError_t(launch_ground(a));
  if (e != hipSuccess) return fail(g->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

}  // extern "C"
