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
int main() {
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
