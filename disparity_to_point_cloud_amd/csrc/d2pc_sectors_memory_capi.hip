// d2pc_sectors_memory_capi.hip -- include/d2pc_sectors.h: the memory session (two record buffers, a parity word and the
// grid's tables in device memory) and its asynchronous calls.  Everything that needs no device -- the refusals, the
// position bound, the coverage -- is d2pc_sectors_memory_plan.hpp's; this file adds the device.
#include <new>
#include <vector>

#include "d2pc_sectors_memory_plan.hpp"
#include "d2pc_sectors_session.hpp"

using namespace d2pc::sectors;

struct d2pc_sectors_memory {
  MemoryPlan plan{};
  int device = 0;
  float *d_table = nullptr;      // half x (c, s), then plan.grid.elev x (ce, se)
  void *d_buffers = nullptr;     // 2 x n_cells records
  uint32_t *d_parity = nullptr;  // which buffer holds the memory; the update kernel flips it
  char err[256] = "";
};

extern "C" {

int d2pc_sectors_memory_create(const d2pc_sectors_config *grid, const d2pc_sectors_memory_config *mcfg, d2pc_sectors_memory **out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  MemoryPlan p;
  const int st = make_memory_plan(grid, mcfg, &p);
  if (st != D2PC_OK) return st;
  if (!device_exists(grid->device_id)) return D2PC_ERR_NO_DEVICE;
  DeviceGuard guard(grid->device_id);
  if (!guard.ok) return D2PC_ERR_NO_DEVICE;
  d2pc_sectors_memory *m = new (std::nothrow) d2pc_sectors_memory();
  if (!m) return D2PC_ERR_OUT_OF_MEMORY;
  m->plan = p, m->device = grid->device_id;
  const size_t n = size_t(p.grid.n_cells);
  std::vector<uint32_t> empty(2 * n * 4, 0u);
  for (size_t i = 0; i < 2 * n; ++i) empty[4 * i + 3] = kEmptyAge;
  const uint32_t zero = 0;
  hipError_t e = upload_table(*grid, p.grid, &m->d_table);
  if (e == hipSuccess) e = hipMalloc(&m->d_buffers, empty.size() * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->d_parity), sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemcpy(m->d_buffers, empty.data(), empty.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->d_parity, &zero, sizeof zero, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)d2pc_sectors_memory_destroy(m);
    return e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE;
  }
  *out = m;
  return D2PC_OK;
}

int d2pc_sectors_memory_destroy(d2pc_sectors_memory *m) {
  if (!m) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(m->device);
  if (m->d_table) (void)hipFree(m->d_table);   // (hipFree waits for the device's work)
  if (m->d_buffers) (void)hipFree(m->d_buffers);
  if (m->d_parity) (void)hipFree(m->d_parity);
  delete m;
  return D2PC_OK;
}

const char *d2pc_sectors_memory_last_error(const d2pc_sectors_memory *m) { return m ? m->err : "null session"; }

void d2pc_sectors_memory_desc_init(d2pc_sectors_memory_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->point_step = 16;
  desc->n_clouds = 1;
}

int d2pc_sectors_memory_desc_check(const d2pc_sectors_config *grid, const d2pc_sectors_memory_config *mcfg,
                                   const d2pc_sectors_memory_desc *desc) {
  MemoryPlan p;
  const int st = make_memory_plan(grid, mcfg, &p);
  return st != D2PC_OK ? st : check_memory_desc(p, desc);
}

int d2pc_sectors_memory_update_device(d2pc_sectors_memory *m, const d2pc_sectors_memory_desc *d, void *stream) {
  if (!m) return D2PC_ERR_INVALID_ARG;
  const int st = check_memory_desc(m->plan, d, m->err, sizeof m->err);
  if (st != D2PC_OK) return st;
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(m->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", m->device);
  MemoryLaunch a;
  a.plan = m->plan;
  a.points = d->points, a.count = d->count, a.nearest = d->nearest, a.step = d->step, a.covered = d->covered;
  a.table = m->d_table, a.buffers = m->d_buffers, a.parity = m->d_parity;
  a.range = d->range, a.distance_cm = d->distance_cm, a.age = d->age, a.records = d->records;
  a.bound = uint32_t(position_bound(*d)), a.step16 = uint32_t(d->point_step / 16);   // (the bound is 0xFFFFFFFF at the most)
  a.stream = stream;   // NULL = HIP's default stream
  const hipError_t e = hipError_t(launch_memory_update(a));
  if (e != hipSuccess) return fail(m->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

int d2pc_sectors_memory_reset_device(d2pc_sectors_memory *m, void *stream) {
  if (!m) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(m->device);
  if (!guard.ok) return fail(m->err, D2PC_ERR_NO_DEVICE, "cannot select device %d", m->device);
  const hipError_t e = hipError_t(launch_memory_reset(m->d_buffers, m->plan.grid.n_cells, stream));
  if (e != hipSuccess) return fail(m->err, D2PC_ERR_DEVICE, "launch failed: %s", hipGetErrorString(e));
  return D2PC_OK;
}

int d2pc_sectors_memory_coverage(const d2pc_sectors_config *grid, const d2pc_sectors_fov *fovs, int n_fovs, uint8_t *covered_host,
                                 int capacity) {
  if (!covered_host || n_fovs < 0 || (n_fovs > 0 && !fovs)) return -D2PC_ERR_INVALID_ARG;
  Plan p;
  const int st = make_plan(grid, &p);
  if (st != D2PC_OK) return -st;
  if (capacity < p.n_cells) return -D2PC_ERR_CAPACITY;
  fill_coverage(*grid, fovs, n_fovs, covered_host);
  return p.n_cells;
}

}  // extern "C"
