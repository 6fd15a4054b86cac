// d2pc_sectors_capi.hip -- include/d2pc_sectors.h: the session (the boundary table and the blocks' slabs in device
// memory; an elevation session's second table behind it) and the one asynchronous call.  Everything that needs no device -- the refusals, rmin2 / rmax2 / inv_h, the
// table's values -- is d2pc_sectors_plan.hpp's; this file adds the device.  libd2pc_sectors.so links the HIP runtime
// only: nothing of d2pc_ctx is needed to read records from device memory.
#include <new>

#include "d2pc_sectors_session.hpp"

using namespace d2pc::sectors;

struct d2pc_sectors {
  d2pc_sectors_config cfg{};
  Plan plan{};
  int device = 0, blocks = 0;
  float *d_table = nullptr;         // half x (c, s), then plan.elev x (ce, se)
  uint64_t *d_slab_keys = nullptr;  // blocks x n_cells
  uint32_t *d_slab_counts = nullptr;
  char err[256] = "";
};

extern "C" {

void d2pc_sectors_config_init(d2pc_sectors_config *cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->n_sectors = 72, cfg->n_layers = 1;
  cfg->azimuth0 = -3.14159265358979323846 / 72.0;
  cfg->r_min = 0.2f, cfg->r_max = INFINITY, cfg->u_min = -INFINITY, cfg->u_max = INFINITY;
  cfg->axes[0] = 3, cfg->axes[1] = -1, cfg->axes[2] = -2;
  cfg->min_count = 1, cfg->no_obstacle_cm = 65535u;
}

int d2pc_sectors_geometry(const d2pc_sectors_config *cfg, d2pc_sectors_geometry_t *out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  Plan p;
  const int st = make_plan(cfg, &p);
  if (st != D2PC_OK) return st;
  fill_geometry(p, out);
  return D2PC_OK;
}

int d2pc_sectors_table(const d2pc_sectors_config *cfg, float *c, float *s, int capacity) {
  if (!c || !s) return -D2PC_ERR_INVALID_ARG;
  Plan p;
  const int st = make_plan(cfg, &p);
  if (st != D2PC_OK) return -st;
  if (capacity < p.half) return -D2PC_ERR_CAPACITY;
  fill_table(*cfg, c, s);
  return p.half;
}

int d2pc_sectors_elevation_table(const d2pc_sectors_config *cfg, float *c, float *s, int capacity) {
  if (!c || !s) return -D2PC_ERR_INVALID_ARG;
  Plan p;
  const int st = make_plan(cfg, &p);
  if (st != D2PC_OK) return -st;
  if (p.layer_kind != D2PC_SECTORS_LAYERS_ELEVATION) return -D2PC_ERR_INVALID_ARG;
  if (capacity < p.elev) return -D2PC_ERR_CAPACITY;
  fill_elevation_table(*cfg, c, s);
  return p.elev;
}

void d2pc_sectors_desc_init(d2pc_sectors_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->point_step = 16;
  desc->n_clouds = 1;
}

int d2pc_sectors_desc_check(const d2pc_sectors_config *cfg, const d2pc_sectors_desc *desc) {
  Plan p;
  const int st = make_plan(cfg, &p);
  return st != D2PC_OK ? st : check_desc(p, desc);
}

int d2pc_sectors_create(const d2pc_sectors_config *cfg, d2pc_sectors **out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  Plan p;
  const int st = make_plan(cfg, &p);
  if (st != D2PC_OK) return st;
  if (!device_exists(cfg->device_id)) return D2PC_ERR_NO_DEVICE;
  DeviceGuard guard(cfg->device_id);
  if (!guard.ok) return D2PC_ERR_NO_DEVICE;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device_id) != hipSuccess || cus < 1) return D2PC_ERR_DEVICE;
  d2pc_sectors *s = new (std::nothrow) d2pc_sectors();
  if (!s) return D2PC_ERR_OUT_OF_MEMORY;
  s->cfg = *cfg, s->plan = p, s->device = cfg->device_id;
  s->blocks = p.blocks_per_cu * cus;
  const size_t cells = size_t(s->blocks) * size_t(p.n_cells);
  hipError_t e = upload_table(*cfg, p, &s->d_table);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_slab_keys), cells * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&s->d_slab_counts), cells * sizeof(uint32_t));
  if (e == hipSuccess) e = hipError_t(prepare_sectors_kernels(p));
  if (e != hipSuccess) {
    (void)d2pc_sectors_destroy(s);
    return e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE;
  }
  *out = s;
  return D2PC_OK;
}

int d2pc_sectors_destroy(d2pc_sectors *s) {
  if (!s) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(s->device);
  if (s->d_table) (void)hipFree(s->d_table);   // (hipFree waits for the device's work)
  if (s->d_slab_keys) (void)hipFree(s->d_slab_keys);
  if (s->d_slab_counts) (void)hipFree(s->d_slab_counts);
  delete s;
  return D2PC_OK;
}

const char *d2pc_sectors_last_error(const d2pc_sectors *s) { return s ? s->err : "null session"; }

int d2pc_sectors_blocks(const d2pc_sectors *s) { return s ? s->blocks : 0; }

int d2pc_sectors_process_device(d2pc_sectors *s, const d2pc_sectors_desc *d, void *stream) {
  if (!s) return D2PC_ERR_INVALID_ARG;
  const int st = check_desc(s->plan, d, s->err, sizeof s->err);
  if (st != D2PC_OK) return st;
  DeviceGuard guard(s->device);
  if (!guard.ok) return fail(s->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", s->device);
  Launch a;
  a.plan = s->plan;
  a.walk = cloud_walk(*d), a.table = s->d_table;
  a.slab_keys = s->d_slab_keys, a.slab_counts = s->d_slab_counts;
  a.range = d->range, a.count = d->count, a.nearest = d->nearest, a.distance_cm = d->distance_cm;
  a.blocks = s->blocks;
  a.stream = stream;   // NULL = HIP's default stream
  const hipError_t e = hipError_t(launch_sectors(a));
  if (e != hipSuccess) return fail(s->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

}  // extern "C"
