// csrc/d2pc_sectors_plan.hpp without a GPU and without HIP: g++ -fsanitize=address,undefined
// (tests/test_sectors_elevation_cpu.py).  The refusals of both layer kinds, the geometry, and both tables filled into
// buffers of exactly their size: a write past one is found.
#include "d2pc_sectors_plan.hpp"
#include <cmath>
#include <vector>
using namespace d2pc::sectors;
static d2pc_sectors_config base(int kind) {
  d2pc_sectors_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.n_sectors = 72; c.n_layers = 1;
  c.r_min = 0.2f; c.r_max = INFINITY; c.u_min = kind ? -0.5f : -INFINITY; c.u_max = kind ? 0.7f : INFINITY;
  c.axes[0] = 3; c.axes[1] = -1; c.axes[2] = -2; c.min_count = 1; c.no_obstacle_cm = 65535u; c.layer_kind = kind; return c; }
static int fails = 0;
static void expect(d2pc_sectors_config c, int want, int line) {
  Plan p; char msg[160] = "";
  const int st = make_plan(&c, &p, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; return; }
  if (st != D2PC_OK) return;
  d2pc_sectors_geometry_t g; fill_geometry(p, &g);
  std::vector<float> cs(size_t(p.half)), sn(size_t(p.half)), ce(size_t(p.elev)), se(size_t(p.elev));   // exact sizes: a write past one is found
  fill_table(c, cs.data(), sn.data());
  if (p.elev) fill_elevation_table(c, ce.data(), se.data());
  if (g.elevation_entries != (c.layer_kind ? c.n_layers + 1 : 0) || g.lds_bytes != size_t(g.n_cells) * 12 + size_t(p.half + p.elev) * 8) {
    printf("line %d: geometry\n", line); ++fails; }
}
#define EXPECT(want, ...) do { d2pc_sectors_config c = base(1); __VA_ARGS__; expect(c, want, __LINE__); } while (0)
// cloud_walk of a descriptor of either kind against the four lines the two capi files held before it
template <class Desc>
static void expect_walk(int n_clouds, size_t stride, size_t cloud_points, int point_step, int line) {
  static const char points[16] = {};
  static const uint32_t counts[3] = {};
  Desc d; memset(&d, 0, sizeof d);
  d.points = points; d.counts = counts; d.n_clouds = n_clouds; d.points_frame_stride_points = stride; d.cloud_points = cloud_points;
  d.point_step = point_step;
  const CloudWalk w = cloud_walk(d);
  const uint64_t want_stride = d.n_clouds > 1 ? uint64_t(d.points_frame_stride_points) : 0;
  const uint32_t want_cp = uint32_t(d.cloud_points), want_n = uint32_t(d.n_clouds), want_step16 = uint32_t(d.point_step / 16);
  const uint32_t want_spc = uint32_t((uint64_t(d.cloud_points) + D2PC_SECTORS_SHARE_POINTS - 1) / D2PC_SECTORS_SHARE_POINTS);
  const uint64_t want_shares = uint64_t(want_spc) * uint64_t(want_n);
  if (w.points != points || w.counts != counts || w.stride != want_stride || w.cloud_points != want_cp || w.n_clouds != want_n ||
      w.step16 != want_step16 || w.shares_per_cloud != want_spc || w.shares != want_shares) {
    printf("line %d: cloud_walk of %d clouds x %zu points\n", line, n_clouds, cloud_points); ++fails; }
}
static void walks() {
  const size_t sizes[4] = {1u, 1024u, 1025u, size_t(0xFFFFFFFFu)};
  const uint32_t shares[4] = {1u, 1u, 2u, 1u << 22};
  for (int i = 0; i < 4; ++i) {
    expect_walk<d2pc_sectors_desc>(1, 0, sizes[i], 16, __LINE__);
    expect_walk<d2pc_sectors_desc>(1, 77, sizes[i], 32, __LINE__);          // (one cloud: its stride is not read)
    expect_walk<d2pc_sectors_ground_desc>(1, 0, sizes[i], 32, __LINE__);
    if (i < 3) expect_walk<d2pc_sectors_desc>(3, 2000, sizes[i], 16, __LINE__), expect_walk<d2pc_sectors_ground_desc>(3, 2000, sizes[i], 16, __LINE__);
    d2pc_sectors_desc d; memset(&d, 0, sizeof d); d.n_clouds = 1; d.cloud_points = sizes[i]; d.point_step = 16;
    if (cloud_walk(d).shares_per_cloud != shares[i]) { printf("line %d: %zu points are not %u shares\n", __LINE__, sizes[i], shares[i]); ++fails; }
  }
  d2pc_sectors_desc d; memset(&d, 0, sizeof d); d.n_clouds = 3; d.points_frame_stride_points = 2000; d.cloud_points = 1025; d.point_step = 32;
  const CloudWalk w = cloud_walk(d);
  if (w.stride != 2000 || w.shares != 6 || w.step16 != 2) { printf("line %d: three clouds with a stride\n", __LINE__); ++fails; }
}
int main() {
  walks();
  expect(base(0), D2PC_OK, __LINE__);
  { d2pc_sectors_config c = base(0); c.n_sectors = 360; c.n_layers = 16; c.u_min = -1.f; c.u_max = 1.f; expect(c, D2PC_OK, __LINE__); }
  { d2pc_sectors_config c = base(0); c.n_layers = 17; expect(c, D2PC_ERR_BAD_SIZE, __LINE__); }
  EXPECT(D2PC_OK, (void)c);
  EXPECT(D2PC_OK, c.n_layers = 64; c.n_sectors = 90; c.u_min = -1.5707964f; c.u_max = 1.5707964f);
  EXPECT(D2PC_OK, c.n_layers = 30; c.n_sectors = 60);
  EXPECT(D2PC_OK, c.n_layers = 16; c.n_sectors = 360);
  EXPECT(D2PC_ERR_INVALID_ARG, c.layer_kind = 2);
  EXPECT(D2PC_ERR_INVALID_ARG, c.layer_kind = -1; c.n_layers = 0);
  EXPECT(D2PC_ERR_INVALID_ARG, c.u_min = NAN);
  EXPECT(D2PC_ERR_INVALID_ARG, c.u_min = 0.8f);
  EXPECT(D2PC_ERR_BAD_SIZE, c.n_layers = 0);
  EXPECT(D2PC_ERR_BAD_SIZE, c.n_layers = 65);
  EXPECT(D2PC_ERR_BAD_SIZE, c.n_layers = INT32_MAX; c.n_sectors = 360);
  EXPECT(D2PC_ERR_BAD_SIZE, c.n_layers = 64; c.n_sectors = 92);
  EXPECT(D2PC_ERR_BAD_SIZE, c.u_max = std::nextafter(1.5707964f, 2.f));
  EXPECT(D2PC_ERR_BAD_SIZE, c.u_min = -INFINITY);
  EXPECT(D2PC_ERR_BAD_SIZE, c.u_max = INFINITY);
  EXPECT(D2PC_ERR_BAD_SIZE, c.u_min = c.u_max);
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
