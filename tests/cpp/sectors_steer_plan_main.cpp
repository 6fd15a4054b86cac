// csrc/d2pc_sectors_steer_plan.hpp without a GPU and without HIP: g++ -fsanitize=address,undefined
// (tests/test_sectors_steer_cpu.py).  The refusals of a steer configuration and of a steer descriptor (the pointers are
// numbers: nothing is dereferenced), the reach tables filled into buffers of exactly their entries (a write past one is
// found), their shape, and the cell of a goal direction.
#include "d2pc_sectors_steer_plan.hpp"
#include <cmath>
#include <vector>
using namespace d2pc::sectors;
static const double kPi = 3.14159265358979323846;
static d2pc_sectors_config grid(int kind, int n = 72, int layers = 0) {
  d2pc_sectors_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.n_sectors = n; c.n_layers = layers ? layers : (kind ? 4 : 1);
  c.r_min = 0.2f; c.r_max = INFINITY; c.u_min = kind ? -0.5f : -INFINITY; c.u_max = kind ? 0.7f : INFINITY;
  c.axes[0] = 3; c.axes[1] = -1; c.axes[2] = -2; c.min_count = 1; c.no_obstacle_cm = 65535u; c.layer_kind = kind; return c; }
static d2pc_sectors_config slabs(int n, int layers, float lo, float hi) { d2pc_sectors_config c = grid(0, n, layers); c.u_min = lo; c.u_max = hi; return c; }
static d2pc_sectors_steer_config steer(int wa = 8, int we = 0) {
  d2pc_sectors_steer_config s; memset(&s, 0, sizeof s); s.struct_size = sizeof s; s.radius = 0.5f; s.max_reach_sectors = wa; s.max_reach_layers = we;
  s.free_cm = 65535u; s.min_clearance_cm = 100u; s.horizon_cm = 1000u; s.w_goal = 16u; s.w_prev = 4u; s.w_near = 1u; return s; }
static const void *at(uintptr_t v) { return reinterpret_cast<const void *>(v); }
static void *out_at(uintptr_t v) { return reinterpret_cast<void *>(v); }
// 72 cells: distance_cm / clearance_cm of 144 bytes, allowed of 72, step of 32, cost of 288, 5 candidates of 40, summary of 16
static const uintptr_t DC = 0x20000000, AL = 0x20001000, ST = 0x20002000, CL = 0x30000000, CO = 0x30001000, CA = 0x30002000, SU = 0x30003000;
static d2pc_sectors_steer_desc good() {
  d2pc_sectors_steer_desc d; memset(&d, 0, sizeof d); d.struct_size = sizeof d; d.n_candidates = 5;
  d.distance_cm = static_cast<const uint16_t *>(at(DC)); d.allowed = static_cast<const uint8_t *>(at(AL));
  d.step = static_cast<const d2pc_sectors_steer_step *>(at(ST)); d.clearance_cm = static_cast<uint16_t *>(out_at(CL));
  d.cost = static_cast<uint32_t *>(out_at(CO)); d.candidates = static_cast<d2pc_sectors_steer_candidate *>(out_at(CA));
  d.summary = static_cast<uint32_t *>(out_at(SU)); return d; }
static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)
static void expect_plan(d2pc_sectors_config c, const d2pc_sectors_steer_config *s, int want, int line) {
  SteerPlan p; char msg[200] = "";
  const int st = make_steer_plan(&c, s, &p, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; return; }
  if (st == D2PC_OK && (p.reach_s_entries != c.n_layers * (s->max_reach_sectors + 1) || p.reach_l_entries != s->max_reach_layers + 1 ||
                        p.lds_bytes < size_t(4 * p.grid.n_cells + 2 * (p.reach_s_entries + p.reach_l_entries)) || p.lds_bytes > 27312 || p.lds_bytes % 16)) {
    printf("line %d: entries or lds\n", line); ++fails; }
}
#define PLAN(want, c, ...) do { d2pc_sectors_steer_config s = steer(); __VA_ARGS__; expect_plan(c, &s, want, __LINE__); } while (0)
static void expect_desc(const d2pc_sectors_config &c, const d2pc_sectors_steer_desc &d, int want, int line) {
  d2pc_sectors_steer_config s = steer();
  SteerPlan p; char msg[200] = "";
  if (make_steer_plan(&c, &s, &p) != D2PC_OK) { printf("line %d: plan\n", line); ++fails; return; }
  const int st = check_steer_desc(p, &d, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; }
}
#define DESC(want, ...) do { d2pc_sectors_steer_desc d = good(); __VA_ARGS__; expect_desc(grid(0), d, want, __LINE__); } while (0)
// 5,760 cells: the same buffers a megabyte apart
static const uintptr_t WDC = 0x40000000, WAL = 0x40100000, WST = 0x40200000, WCL = 0x50000000, WCO = 0x50100000, WCA = 0x50200000, WSU = 0x50300000;
static d2pc_sectors_steer_desc wide() {
  d2pc_sectors_steer_desc d = good();
  d.distance_cm = static_cast<const uint16_t *>(at(WDC)); d.allowed = static_cast<const uint8_t *>(at(WAL));
  d.step = static_cast<const d2pc_sectors_steer_step *>(at(WST)); d.clearance_cm = static_cast<uint16_t *>(out_at(WCL));
  d.cost = static_cast<uint32_t *>(out_at(WCO)); d.candidates = static_cast<d2pc_sectors_steer_candidate *>(out_at(WCA));
  d.summary = static_cast<uint32_t *>(out_at(WSU)); return d; }
#define WIDE(want, ...) do { d2pc_sectors_steer_desc d = wide(); __VA_ARGS__; expect_desc(slabs(360, 16, 0.f, 4.f), d, want, __LINE__); } while (0)
// the tables into buffers of exactly their entries; -> false where their shape is not the specification's
static bool reach_ok(const d2pc_sectors_config &c, const d2pc_sectors_steer_config &s) {
  SteerPlan p;
  if (make_steer_plan(&c, &s, &p) != D2PC_OK) return false;
  std::vector<uint16_t> rs(size_t(p.reach_s_entries), 7), rl(size_t(p.reach_l_entries), 7);
  fill_reach(c, s, rs.data(), rl.data());
  bool ok = rl[0] == 65535;
  for (int k = 1; k <= p.we; ++k) ok = ok && rl[size_t(k)] <= 65534 && (k == 1 || rl[size_t(k)] <= rl[size_t(k - 1)]);
  for (int i = 0; i < c.n_layers; ++i) {
    const uint16_t *row = rs.data() + size_t(i) * size_t(p.wa + 1);
    ok = ok && row[0] == 65535;
    for (int k = 1; k <= p.wa; ++k) ok = ok && row[k] <= 65534 && row[k] >= uint16_t(100.0 * double(s.radius)) && (k == 1 || row[k] <= row[k - 1]);
  }
  return ok;
}
static void expect_cell(const d2pc_sectors_config &c, double yaw, double third, int want, uint32_t sector, uint32_t layer, int line) {
  uint32_t s = 77777, l = 77777; char msg[200] = "";
  const int st = steer_goal_cell(c, yaw, third, &s, &l, msg, sizeof msg);
  if (st != want || (st == D2PC_OK && (s != sector || l != layer)) || (st != D2PC_OK && (!msg[0] || s != 77777 || l != 77777))) {
    printf("line %d: status %d (%u, %u), not %d (%u, %u) (%s)\n", line, st, s, l, want, sector, layer, msg); ++fails; }
}
int main() {
  // ---- the configuration: the grid's refusals first, then INVALID_ARG, then BAD_SIZE
  PLAN(D2PC_OK, grid(0), (void)s);
  PLAN(D2PC_OK, grid(1), s.max_reach_layers = 3);
  PLAN(D2PC_OK, grid(0), s.max_reach_sectors = 0);
  PLAN(D2PC_OK, grid(0), s.max_reach_sectors = 32; s.w_goal = s.w_prev = s.w_near = 4095; s.free_cm = s.min_clearance_cm = s.horizon_cm = 65535);
  PLAN(D2PC_OK, grid(0), s.free_cm = s.min_clearance_cm = s.horizon_cm = 0; s.w_goal = s.w_prev = s.w_near = 0);
  PLAN(D2PC_OK, grid(1, 90, 64), s.max_reach_sectors = 32; s.max_reach_layers = 16);     // the largest tables
  PLAN(D2PC_OK, grid(0, 8), s.max_reach_sectors = 4);
  PLAN(D2PC_OK, slabs(12, 4, -2.f, 2.f), s.max_reach_sectors = 6; s.max_reach_layers = 3);
  expect_plan(grid(0), nullptr, D2PC_ERR_INVALID_ARG, __LINE__);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.struct_size = 44);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.radius = 0.f);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.radius = -0.5f);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.radius = NAN);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.radius = INFINITY);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.w_goal = 4096);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.w_prev = 4096);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.w_near = 0xFFFFFFFFu);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.free_cm = 65536);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.min_clearance_cm = 65536);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.horizon_cm = 65536);
  PLAN(D2PC_ERR_INVALID_ARG, grid(0), s.radius = 0.f; s.max_reach_sectors = 99);       // INVALID_ARG before BAD_SIZE
  PLAN(D2PC_ERR_BAD_SIZE, grid(0), s.max_reach_sectors = 33);
  PLAN(D2PC_ERR_BAD_SIZE, grid(0), s.max_reach_sectors = -1);
  PLAN(D2PC_ERR_BAD_SIZE, grid(1, 90, 64), s.max_reach_layers = 17);
  PLAN(D2PC_ERR_BAD_SIZE, grid(1), s.max_reach_layers = -1);
  PLAN(D2PC_ERR_BAD_SIZE, grid(0, 8), s.max_reach_sectors = 5);                        // n / 2 is 4
  PLAN(D2PC_ERR_BAD_SIZE, grid(0), s.max_reach_layers = 1);                            // one layer
  PLAN(D2PC_ERR_BAD_SIZE, grid(1), s.max_reach_layers = 4);                            // L - 1 is 3
  PLAN(D2PC_ERR_INVALID_ARG, grid(0, 71), s.max_reach_sectors = 99);                   // the grid's refusal, with its status
  PLAN(D2PC_ERR_BAD_SIZE, grid(0, 72, 17), s.radius = 0.f);
  // ---- the descriptor
  DESC(D2PC_OK, (void)d);
  DESC(D2PC_OK, d.allowed = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.struct_size = 56);
  DESC(D2PC_ERR_INVALID_ARG, d.distance_cm = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.step = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.clearance_cm = nullptr; d.cost = nullptr; d.candidates = nullptr; d.summary = nullptr);
  DESC(D2PC_OK, d.cost = nullptr; d.candidates = nullptr; d.summary = nullptr);
  DESC(D2PC_OK, d.clearance_cm = nullptr; d.candidates = nullptr; d.summary = nullptr);
  DESC(D2PC_OK, d.clearance_cm = nullptr; d.cost = nullptr; d.summary = nullptr);
  DESC(D2PC_OK, d.clearance_cm = nullptr; d.cost = nullptr; d.candidates = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 0);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 33);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = -1);
  DESC(D2PC_OK, d.n_candidates = 32);
  DESC(D2PC_OK, d.n_candidates = 0; d.candidates = nullptr);                          // not looked at without candidates
  DESC(D2PC_ERR_INVALID_ARG, d.distance_cm = static_cast<const uint16_t *>(at(DC + 1)));
  DESC(D2PC_ERR_INVALID_ARG, d.step = static_cast<const d2pc_sectors_steer_step *>(at(ST + 2)));
  DESC(D2PC_ERR_INVALID_ARG, d.clearance_cm = static_cast<uint16_t *>(out_at(CL + 1)));
  DESC(D2PC_ERR_INVALID_ARG, d.cost = static_cast<uint32_t *>(out_at(CO + 2)));
  DESC(D2PC_ERR_INVALID_ARG, d.candidates = static_cast<d2pc_sectors_steer_candidate *>(out_at(CA + 4)));
  DESC(D2PC_ERR_INVALID_ARG, d.summary = static_cast<uint32_t *>(out_at(SU + 2)));
  DESC(D2PC_OK, d.distance_cm = static_cast<const uint16_t *>(at(DC + 2)); d.allowed = static_cast<const uint8_t *>(at(AL + 1));
       d.step = static_cast<const d2pc_sectors_steer_step *>(at(ST + 4)); d.candidates = static_cast<d2pc_sectors_steer_candidate *>(out_at(CA + 8)));
  // overlaps: every output over the first and the last byte of every other buffer
  { const uintptr_t base[7] = {DC, AL, ST, CL, CO, CA, SU}; const size_t size[7] = {144, 72, 32, 144, 288, 40, 16};
    for (int o = 3; o < 7; ++o)
      for (int b = 0; b < 7; ++b) {
        if (b == o) continue;
        const size_t al = o == 5 ? 8 : (o == 3 ? 2 : 4);             // the output's alignment: steps of it keep the pointer aligned
        const uintptr_t first = base[b] - size[o] + al, clear_lo = base[b] - size[o];
        const uintptr_t last = (base[b] + size[b] - 1) / al * al, clear_hi = (base[b] + size[b] + al - 1) / al * al;
        for (int k = 0; k < 4; ++k) {
          d2pc_sectors_steer_desc d = good();
          const uintptr_t v = k == 0 ? first : k == 1 ? clear_lo : k == 2 ? last : clear_hi;
          if (o == 3) d.clearance_cm = static_cast<uint16_t *>(out_at(v));
          if (o == 4) d.cost = static_cast<uint32_t *>(out_at(v));
          if (o == 5) d.candidates = static_cast<d2pc_sectors_steer_candidate *>(out_at(v));
          if (o == 6) d.summary = static_cast<uint32_t *>(out_at(v));
          expect_desc(grid(0), d, k % 2 == 0 ? D2PC_ERR_INVALID_ARG : D2PC_OK, __LINE__ * 1000 + o * 100 + b * 10 + k);
        }
      }
  }
  DESC(D2PC_OK, d.allowed = nullptr; d.summary = static_cast<uint32_t *>(out_at(AL + 68)));   // a buffer that is not given overlaps nothing
  DESC(D2PC_OK, d.n_candidates = 1; d.summary = static_cast<uint32_t *>(out_at(CA + 8)));      // the candidates' extent is n_candidates
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 2; d.summary = static_cast<uint32_t *>(out_at(CA + 8)));
  // the extents follow the session's cells: 5,760
  WIDE(D2PC_OK, (void)d);
  WIDE(D2PC_ERR_INVALID_ARG, d.cost = static_cast<uint32_t *>(out_at(WDC + 2 * 5760 - 4)));
  WIDE(D2PC_OK, d.cost = static_cast<uint32_t *>(out_at(WDC + 2 * 5760)));
  WIDE(D2PC_ERR_INVALID_ARG, d.summary = static_cast<uint32_t *>(out_at(WAL + 5760 - 4)));
  WIDE(D2PC_OK, d.summary = static_cast<uint32_t *>(out_at(WAL + 5760)));
  WIDE(D2PC_ERR_INVALID_ARG, d.summary = static_cast<uint32_t *>(out_at(WCL + 2 * 5760 - 4)));
  WIDE(D2PC_OK, d.summary = static_cast<uint32_t *>(out_at(WCL + 2 * 5760)));
  WIDE(D2PC_ERR_INVALID_ARG, d.clearance_cm = static_cast<uint16_t *>(out_at(WCO - 2 * 5760 + 2)));
  WIDE(D2PC_OK, d.clearance_cm = static_cast<uint16_t *>(out_at(WCO - 2 * 5760)));
  WIDE(D2PC_ERR_INVALID_ARG, d.summary = static_cast<uint32_t *>(out_at(WCO + 4 * 5760 - 4)));
  WIDE(D2PC_OK, d.summary = static_cast<uint32_t *>(out_at(WCO + 4 * 5760)));
  WIDE(D2PC_ERR_INVALID_ARG, d.cost = static_cast<uint32_t *>(out_at(WST - 4 * 5760 + 4)));
  WIDE(D2PC_OK, d.cost = static_cast<uint32_t *>(out_at(WST - 4 * 5760)));
  // ---- the reach tables, filled into exactly their capacity
  { d2pc_sectors_steer_config s = steer(8, 0); CHECK(reach_ok(grid(0), s)); }
  { d2pc_sectors_steer_config s = steer(0, 0); CHECK(reach_ok(grid(0), s)); }
  { d2pc_sectors_steer_config s = steer(32, 16); s.radius = 1.0f; d2pc_sectors_config c = grid(1, 90, 64); c.u_min = -1.2f; c.u_max = 1.2f; CHECK(reach_ok(c, s)); }
  { d2pc_sectors_steer_config s = steer(8, 4); d2pc_sectors_config c = grid(1, 60, 30); c.u_min = -kHalfPi; c.u_max = kHalfPi; CHECK(reach_ok(c, s));
    SteerPlan p; std::vector<uint16_t> rs(30 * 9), rl(5);
    CHECK(make_steer_plan(&c, &s, &p) == D2PC_OK); fill_reach(c, s, rs.data(), rl.data());
    CHECK(rs[1] < 65534 && rs[1] > 18000 && std::abs(int(rs[1]) - int(rs[29 * 9 + 1])) <= 1);   // 50 / sin(3 degrees x 0.052), at both ends of a symmetric band
    { d2pc_sectors_steer_config wide = steer(8, 4); wide.radius = 2.0f; std::vector<uint16_t> ws(30 * 9), wl(5); fill_reach(c, wide, ws.data(), wl.data());
      CHECK(ws[1] == 65534 && ws[29 * 9 + 1] == 65534 && ws[15 * 9 + 1] < 65534); }   // next to the poles the clamp
    CHECK(rs[15 * 9 + 1] == uint16_t(std::floor(50.0 / std::sin(0.5 * (2 * kPi / 60) * std::cos((double(-kHalfPi) + 15.0 * (2.0 * double(kHalfPi)) / 30.0) + (2.0 * double(kHalfPi)) / 60.0))))); }
  { d2pc_sectors_steer_config s = steer(3, 2); s.radius = 0.75f; const d2pc_sectors_config c = slabs(8, 3, -1.5f, 1.5f); CHECK(reach_ok(c, s));
    std::vector<uint16_t> rs(3 * 4), rl(3); fill_reach(c, s, rs.data(), rl.data());
    CHECK(rl[1] == 65534 && rl[2] == 0);                              // half a slab (0.5) is below the radius, one and a half is not
    CHECK(rs[3] == 75 && rs[7] == 75 && rs[2] == uint16_t(std::floor(75.0 / std::sin(1.5 * kPi / 4)))); }   // 2.5 x 45 degrees: beyond pi / 2
  CHECK(steer_reach(0.5, 0.0) == 65534 && steer_reach(0.5, -1.0) == 65534 && steer_reach(0.5, 1e-9) == 65534 && steer_reach(700.0, 2.0) == 65534);
  CHECK(steer_reach(0.5, kPi / 6) == 99 || steer_reach(0.5, kPi / 6) == 100);   // 50 / sin(30 degrees), whichever side of 100 the sine falls
  // ---- the cell of a goal direction
  { const d2pc_sectors_config c = grid(0); const double a = 2 * kPi / 72;        // azimuth0 = 0
    expect_cell(c, 0.5 * a, 0.0, D2PC_OK, 0, 0, __LINE__);
    expect_cell(c, 71.5 * a, 0.0, D2PC_OK, 71, 0, __LINE__);
    expect_cell(c, -0.5 * a, 0.0, D2PC_OK, 71, 0, __LINE__);
    expect_cell(c, -1e-18, 0.0, D2PC_OK, 71, 0, __LINE__);                          // -1e-18 + 2 pi rounds to a whole turn
    expect_cell(c, 10.5 * a + 8 * kPi, 0.9, D2PC_OK, 10, 0, __LINE__);
    expect_cell(c, 10.5 * a - 6 * kPi, 0.0, D2PC_OK, 10, 0, __LINE__);
    expect_cell(c, 1.0, 1.0, D2PC_ERR_INVALID_ARG, 0, 0, __LINE__);                  // one layer: 0 <= layer < 1
    expect_cell(c, 1.0, -0.5, D2PC_ERR_INVALID_ARG, 0, 0, __LINE__);
    expect_cell(c, NAN, 0.0, D2PC_ERR_INVALID_ARG, 0, 0, __LINE__);
    expect_cell(c, INFINITY, 0.0, D2PC_ERR_INVALID_ARG, 0, 0, __LINE__);
    expect_cell(c, 0.0, NAN, D2PC_ERR_INVALID_ARG, 0, 0, __LINE__); }
  { const d2pc_sectors_config c = slabs(12, 4, -2.f, 2.f);
    expect_cell(c, 0.1, 3.0, D2PC_OK, 0, 3, __LINE__); expect_cell(c, 0.1, 3.99, D2PC_OK, 0, 3, __LINE__);
    expect_cell(c, 0.1, 4.0, D2PC_ERR_INVALID_ARG, 0, 0, __LINE__); }
  { d2pc_sectors_config c = grid(1); c.azimuth0 = 0.3;                           // 72 x 4, the band -0.5 .. 0.7: layers of 0.3
    expect_cell(c, 0.3 + 1e-9, -0.5, D2PC_OK, 0, 0, __LINE__);
    expect_cell(c, 0.3 - 1e-9, -0.21, D2PC_OK, 71, 0, __LINE__);
    expect_cell(c, 0.3 + kPi, -0.19, D2PC_OK, 36, 1, __LINE__);
    expect_cell(c, 0.0, 0.69, D2PC_OK, 68, 3, __LINE__);
    expect_cell(c, 0.0, double(c.u_max), D2PC_ERR_INVALID_ARG, 0, 0, __LINE__);
    expect_cell(c, 0.0, -0.51, D2PC_ERR_INVALID_ARG, 0, 0, __LINE__); }
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
