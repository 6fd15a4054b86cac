// csrc/d2pc_sectors_memory_plan.hpp without a GPU and without HIP: g++ -fsanitize=address,undefined
// (tests/test_sectors_memory_cpu.py).  The refusals of a memory configuration and of a memory descriptor (the pointers are
// numbers: nothing is dereferenced), the position bound, and the coverage filled into a buffer of exactly n_cells bytes: a
// write past it is found.
#include "d2pc_sectors_memory_plan.hpp"
#include <cmath>
#include <vector>
using namespace d2pc::sectors;
static d2pc_sectors_config grid(int kind) {
  d2pc_sectors_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.n_sectors = 72; c.n_layers = kind ? 4 : 1;
  c.r_min = 0.2f; c.r_max = INFINITY; c.u_min = kind ? -0.5f : -INFINITY; c.u_max = kind ? 0.7f : INFINITY;
  c.axes[0] = 3; c.axes[1] = -1; c.axes[2] = -2; c.min_count = 1; c.no_obstacle_cm = 65535u; c.layer_kind = kind; return c; }
static d2pc_sectors_memory_config mem(uint32_t max_age) {
  d2pc_sectors_memory_config m; memset(&m, 0, sizeof m); m.struct_size = sizeof m; m.max_age = max_age; return m; }
static const void *at(uintptr_t v) { return reinterpret_cast<const void *>(v); }
static void *out_at(uintptr_t v) { return reinterpret_cast<void *>(v); }
// 72 cells: count / nearest / range / age of 288 bytes, distance_cm of 144, covered of 72, records of 1,152, step of 64
static const uintptr_t P = 0x10000000, CN = 0x20000000, NR = 0x20001000, ST = 0x20002000, CV = 0x20003000, RG = 0x30000000,
                       CM = 0x30001000, AG = 0x30002000, RC = 0x30003000;
static d2pc_sectors_memory_desc good() {
  d2pc_sectors_memory_desc d; memset(&d, 0, sizeof d); d.struct_size = sizeof d; d.point_step = 16; d.n_clouds = 1;
  d.points = at(P); d.cloud_points = 1000; d.count = static_cast<const uint32_t *>(at(CN)); d.nearest = static_cast<const uint32_t *>(at(NR));
  d.step = static_cast<const d2pc_sectors_memory_step *>(at(ST)); d.covered = static_cast<const uint8_t *>(at(CV));
  d.range = static_cast<float *>(out_at(RG)); d.distance_cm = static_cast<uint16_t *>(out_at(CM)); d.age = static_cast<uint32_t *>(out_at(AG));
  d.records = out_at(RC); return d; }
static int fails = 0;
static void expect_plan(d2pc_sectors_config c, const d2pc_sectors_memory_config *m, int want, int line) {
  MemoryPlan p; char msg[160] = "";
  const int st = make_memory_plan(&c, m, &p, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; return; }
  if (st == D2PC_OK && p.lds_bytes != size_t(p.grid.n_cells) * 8 + size_t(p.grid.half + p.grid.elev) * 8) { printf("line %d: lds\n", line); ++fails; }
}
static void expect_desc(const d2pc_sectors_memory_desc &d, int want, int line) {
  d2pc_sectors_config c = grid(0); d2pc_sectors_memory_config m = mem(5000);
  MemoryPlan p; char msg[160] = "";
  if (make_memory_plan(&c, &m, &p) != D2PC_OK) { printf("line %d: plan\n", line); ++fails; return; }
  const int st = check_memory_desc(p, &d, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; }
}
#define DESC(want, ...) do { d2pc_sectors_memory_desc d = good(); __VA_ARGS__; expect_desc(d, want, __LINE__); } while (0)
int main() {
  { d2pc_sectors_memory_config m = mem(0); expect_plan(grid(0), &m, D2PC_OK, __LINE__); expect_plan(grid(1), &m, D2PC_OK, __LINE__); }
  { d2pc_sectors_memory_config m = mem(0xFFFFFFFEu); expect_plan(grid(0), &m, D2PC_OK, __LINE__); }
  { d2pc_sectors_memory_config m = mem(0xFFFFFFFFu); expect_plan(grid(0), &m, D2PC_ERR_INVALID_ARG, __LINE__); }
  { d2pc_sectors_memory_config m = mem(7); m.struct_size = 12; expect_plan(grid(0), &m, D2PC_ERR_INVALID_ARG, __LINE__); }
  expect_plan(grid(0), nullptr, D2PC_ERR_INVALID_ARG, __LINE__);
  { d2pc_sectors_memory_config m = mem(7); d2pc_sectors_config c = grid(0); c.n_sectors = 71; expect_plan(c, &m, D2PC_ERR_INVALID_ARG, __LINE__);
    c = grid(0); c.n_layers = 17; expect_plan(c, &m, D2PC_ERR_BAD_SIZE, __LINE__);
    c = grid(1); c.n_layers = 64; c.n_sectors = 92; expect_plan(c, &m, D2PC_ERR_BAD_SIZE, __LINE__);
    c = grid(1); c.n_layers = 64; c.n_sectors = 90; expect_plan(c, &m, D2PC_OK, __LINE__);
    c = grid(0); c.n_sectors = 360; c.n_layers = 16; c.u_min = -1.f; c.u_max = 1.f; expect_plan(c, &m, D2PC_OK, __LINE__);
    c = grid(0); c.n_layers = 2; expect_plan(c, nullptr, D2PC_ERR_BAD_SIZE, __LINE__); }   // the grid's refusal comes first
  DESC(D2PC_OK, (void)d);
  DESC(D2PC_OK, d.point_step = 32; d.covered = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.struct_size = 96);
  DESC(D2PC_ERR_INVALID_ARG, d.point_step = 24);
  DESC(D2PC_ERR_INVALID_ARG, d.n_clouds = 0);
  DESC(D2PC_ERR_INVALID_ARG, d.n_clouds = 65536; d.points_frame_stride_points = 1000);
  DESC(D2PC_ERR_INVALID_ARG, d.points = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.count = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.nearest = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.step = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.range = nullptr; d.distance_cm = nullptr; d.age = nullptr; d.records = nullptr);
  DESC(D2PC_OK, d.range = nullptr; d.distance_cm = nullptr; d.age = nullptr);
  DESC(D2PC_OK, d.distance_cm = nullptr; d.age = nullptr; d.records = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.points = at(P + 8));
  DESC(D2PC_ERR_INVALID_ARG, d.records = out_at(RC + 8));
  DESC(D2PC_ERR_INVALID_ARG, d.count = static_cast<const uint32_t *>(at(CN + 2)));
  DESC(D2PC_ERR_INVALID_ARG, d.step = static_cast<const d2pc_sectors_memory_step *>(at(ST + 2)));
  DESC(D2PC_ERR_INVALID_ARG, d.distance_cm = static_cast<uint16_t *>(out_at(CM + 1)));
  DESC(D2PC_ERR_INVALID_ARG, d.age = static_cast<uint32_t *>(out_at(AG + 2)));
  DESC(D2PC_ERR_BAD_SIZE, d.cloud_points = 0);
  DESC(D2PC_ERR_BAD_SIZE, d.cloud_points = size_t(1) << 32; d.points = at(uintptr_t(1) << 44));
  DESC(D2PC_OK, d.cloud_points = (size_t(1) << 32) - 1; d.points = at(uintptr_t(1) << 44));
  DESC(D2PC_ERR_BAD_SIZE, d.n_clouds = 3; d.points_frame_stride_points = 999);
  DESC(D2PC_OK, d.n_clouds = 3; d.points_frame_stride_points = 1000);
  DESC(D2PC_ERR_BAD_SIZE, d.points = at(uintptr_t(1) << 44); d.n_clouds = 2; d.cloud_points = size_t(1) << 30; d.points_frame_stride_points = size_t(3) << 30);
  DESC(D2PC_OK, d.points = at(uintptr_t(1) << 44); d.n_clouds = 2; d.cloud_points = size_t(1) << 30; d.points_frame_stride_points = (size_t(3) << 30) - 1);
  DESC(D2PC_ERR_BAD_SIZE, d.n_clouds = 2; d.cloud_points = 5; d.points_frame_stride_points = size_t(1) << 63);
  // overlaps: an output over the records' last byte, over each input's last byte, over another output
  DESC(D2PC_ERR_INVALID_ARG, d.range = static_cast<float *>(out_at(P + 16 * 1000 - 4)));
  DESC(D2PC_OK, d.range = static_cast<float *>(out_at(P + 16 * 1000)));
  DESC(D2PC_ERR_INVALID_ARG, d.age = static_cast<uint32_t *>(out_at(CN + 284)));
  DESC(D2PC_OK, d.age = static_cast<uint32_t *>(out_at(CN + 288)));
  DESC(D2PC_ERR_INVALID_ARG, d.age = static_cast<uint32_t *>(out_at(NR + 284)));
  DESC(D2PC_ERR_INVALID_ARG, d.distance_cm = static_cast<uint16_t *>(out_at(ST + 62)));
  DESC(D2PC_OK, d.distance_cm = static_cast<uint16_t *>(out_at(ST + 64)));
  DESC(D2PC_ERR_INVALID_ARG, d.distance_cm = static_cast<uint16_t *>(out_at(CV + 70)));
  DESC(D2PC_OK, d.distance_cm = static_cast<uint16_t *>(out_at(CV + 72)));
  DESC(D2PC_OK, d.covered = nullptr; d.distance_cm = static_cast<uint16_t *>(out_at(CV + 70)));
  DESC(D2PC_ERR_INVALID_ARG, d.records = out_at(RG + 272));
  DESC(D2PC_OK, d.records = out_at(RG + 288));
  DESC(D2PC_ERR_INVALID_ARG, d.age = static_cast<uint32_t *>(out_at(RC + 1148)));
  DESC(D2PC_OK, d.age = static_cast<uint32_t *>(out_at(RC + 1152)));
  { d2pc_sectors_memory_desc d = good(); d.n_clouds = 3; d.points_frame_stride_points = 1007;
    if (position_bound(d) != 2 * 1007 + 1000) { printf("line %d: bound\n", __LINE__); ++fails; }
    d.n_clouds = 1; if (position_bound(d) != 1000) { printf("line %d: bound\n", __LINE__); ++fails; } }
  for (int kind = 0; kind < 2; ++kind) {   // the coverage into exactly n_cells bytes
    const d2pc_sectors_config c = grid(kind);
    const d2pc_sectors_fov fov[2] = {{0.1, 0.05, 1.5, 0.6, 0.02}, {3.0, 0.0, 1.0, 1.0, 0.0}};
    std::vector<uint8_t> cov(size_t(c.n_sectors) * size_t(c.n_layers), 7);
    fill_coverage(c, fov, 2, cov.data());
    size_t ones = 0;
    for (uint8_t v : cov) { if (v > 1) { printf("line %d: coverage byte %d\n", __LINE__, int(v)); ++fails; } ones += v; }
    if (ones == 0 || ones == cov.size()) { printf("line %d: coverage of %zu cells\n", __LINE__, ones); ++fails; }
    fill_coverage(c, nullptr, 0, cov.data());
    for (uint8_t v : cov) if (v) { printf("line %d: no field of view covers a cell\n", __LINE__); ++fails; break; }
  }
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
