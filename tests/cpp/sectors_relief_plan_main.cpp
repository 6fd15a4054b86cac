// csrc/d2pc_sectors_relief_plan.hpp without a GPU and without the device runtime: g++ -fsanitize=address,undefined
// (tests/test_sectors_relief_cpu.py).  The refusals of the three configurations in their documented order (the slope
// geometry's first: the ground's, the slope's, the table's size; then the depth's), the sizes of the state block and the
// blocks of the window launch, and the refusals of a relief descriptor, the overlap with the session's state included (the
// pointers are numbers: nothing is dereferenced).
#include "d2pc_sectors_relief_plan.hpp"
using namespace d2pc::sectors;
static d2pc_sectors_ground_config ground(int n_a = 16, int n_b = 16) {
  d2pc_sectors_ground_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.n_a = n_a; c.n_b = n_b; c.cell_size = 0.5f; c.quantum = 0.001953125f;
  c.axes[0] = 1; c.axes[1] = 2; c.axes[2] = 3; c.min_count = 4; c.max_spread_q2 = 625; c.max_step_q = 50; c.window = 1;
  c.w_dist = 1; c.w_rough = 1; c.rough_cap = 65535; return c; }
static d2pc_sectors_slope_config slope(int sub = 8) {
  d2pc_sectors_slope_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.sub = sub; c.max_slope = 0.25f; return c; }
static d2pc_sectors_terrain_config terrain(int depth = 8) {
  d2pc_sectors_terrain_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.depth = depth; return c; }
// 256 cells: the six inputs, then the thirteen outputs
static const int N_IN = 6, N_OUT = 13, N_BUF = 19;
static const uintptr_t BASE[N_BUF] = {0x20000000, 0x20100000, 0x20200000, 0x20300000, 0x20400000, 0x20500000, 0x30000000, 0x30100000, 0x30200000, 0x30300000,
                                      0x30400000, 0x30500000, 0x30600000, 0x30700000, 0x30800000, 0x30900000, 0x30A00000, 0x30B00000, 0x30C00000};
static const size_t SIZE[N_BUF] = {80, 1024, 2048, 2048, 14336, 256, 1024, 2048, 2048, 14336, 1024, 1024, 1024, 1024, 256, 256, 40, 16, 16};
static const size_t ALIGN[N_BUF] = {4, 4, 8, 8, 8, 1, 4, 8, 8, 8, 4, 4, 4, 4, 1, 1, 8, 4, 4};
static void set_buf(d2pc_sectors_relief_desc &d, int b, uintptr_t v) {
  void *q = v ? reinterpret_cast<void *>(v) : nullptr;
  switch (b) {
    case 0: d.step = static_cast<const d2pc_sectors_ground_step *>(q); break;
    case 1: d.frame_count = static_cast<const uint32_t *>(q); break;
    case 2: d.frame_sum = static_cast<const int64_t *>(q); break;
    case 3: d.frame_sum2 = static_cast<const uint64_t *>(q); break;
    case 4: d.frame_moments = static_cast<const int64_t *>(q); break;
    case 5: d.allowed = static_cast<const uint8_t *>(q); break;
    case 6: d.count = static_cast<uint32_t *>(q); break;
    case 7: d.sum = static_cast<int64_t *>(q); break;
    case 8: d.sum2 = static_cast<uint64_t *>(q); break;
    case 9: d.moments = static_cast<int64_t *>(q); break;
    case 10: d.slope_a = static_cast<float *>(q); break;
    case 11: d.slope_b = static_cast<float *>(q); break;
    case 12: d.level_q = static_cast<int32_t *>(q); break;
    case 13: d.resid_q2 = static_cast<uint32_t *>(q); break;
    case 14: d.flat = static_cast<uint8_t *>(q); break;
    case 15: d.site = static_cast<uint8_t *>(q); break;
    case 16: d.candidates = static_cast<d2pc_sectors_ground_candidate *>(q); break;
    case 17: d.summary = static_cast<uint32_t *>(q); break;
    default: d.status = static_cast<uint32_t *>(q); break;
  }
}
static d2pc_sectors_relief_desc good() {
  d2pc_sectors_relief_desc d; memset(&d, 0, sizeof d); d.struct_size = sizeof d; d.n_candidates = 5;
  for (int b = 0; b < N_BUF; ++b) set_buf(d, b, BASE[b]);
  return d; }
static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)
static void expect_plan(const d2pc_sectors_ground_config *g, const d2pc_sectors_slope_config *s, const d2pc_sectors_terrain_config *c, int want,
                        const char *word, int line) {
  ReliefPlan p; char msg[256] = "";
  const int st = make_relief_plan(g, s, c, &p, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && (!msg[0] || (word && !strstr(msg, word))))) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; return; }
  const size_t n = st == D2PC_OK ? size_t(p.slope.ground.n_cells) : 0;
  if (st == D2PC_OK && (p.depth != c->depth || p.slot_bytes % 16 || p.slot_bytes < 76 * n || p.slot_bytes >= 76 * n + 16 ||
                        p.state_bytes != 256 + size_t(p.depth) * p.slot_bytes || size_t(p.blocks) != (n + 15) / 16)) { printf("line %d: sizes\n", line); ++fails; }
}
#define PLAN(want, word, ...) do { d2pc_sectors_ground_config g = ground(); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain(); \
                                   __VA_ARGS__; expect_plan(&g, &s, &c, want, word, __LINE__); } while (0)
static void expect_desc(const d2pc_sectors_relief_desc &d, int want, int line, int n_a = 16, int n_b = 16) {
  d2pc_sectors_ground_config g = ground(n_a, n_b); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain();
  ReliefPlan p; char msg[256] = "";
  if (make_relief_plan(&g, &s, &c, &p) != D2PC_OK) { printf("line %d: plan\n", line); ++fails; return; }
  const int st = check_relief_desc(p, &d, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; }
}
#define DESC(want, ...) do { d2pc_sectors_relief_desc d = good(); __VA_ARGS__; expect_desc(d, want, __LINE__); } while (0)
int main() {
  // ---- the configurations, in the documented order
  PLAN(D2PC_OK, nullptr, (void)c);
  PLAN(D2PC_OK, nullptr, c.depth = 1);
  PLAN(D2PC_OK, nullptr, c.depth = 16; g.n_a = 46; g.n_b = 46);
  PLAN(D2PC_OK, nullptr, c.depth = 3; g.n_a = 5; g.n_b = 3);
  PLAN(D2PC_OK, nullptr, g.n_a = 43; g.n_b = 50);                                       // 2,150 cells pass
  PLAN(D2PC_ERR_BAD_SIZE, "2155", g.n_a = 47; g.n_b = 46);                              // 2,162 do not
  { d2pc_sectors_ground_config g = ground(); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain();
    expect_plan(nullptr, &s, &c, D2PC_ERR_INVALID_ARG, "ground", __LINE__); expect_plan(&g, nullptr, &c, D2PC_ERR_INVALID_ARG, "slope", __LINE__);
    expect_plan(&g, &s, nullptr, D2PC_ERR_INVALID_ARG, "terrain", __LINE__); expect_plan(&g, nullptr, nullptr, D2PC_ERR_INVALID_ARG, "slope", __LINE__); }
  PLAN(D2PC_ERR_INVALID_ARG, "quantum", g.quantum = 0.f; s.sub = 3; c.depth = 0);      // the ground's first
  PLAN(D2PC_ERR_BAD_SIZE, "cells", g.n_a = 65; s.struct_size = 0; c.struct_size = 0);
  PLAN(D2PC_ERR_INVALID_ARG, "sub", s.sub = 3; c.depth = 0);                            // then the slope's, before the depth's BAD_SIZE
  PLAN(D2PC_ERR_INVALID_ARG, "sub", s.sub = 3; g.n_a = 64; g.n_b = 64);                 // ... and before its own table size
  PLAN(D2PC_ERR_INVALID_ARG, "max_slope", s.max_slope = -1.f; c.depth = 17);
  PLAN(D2PC_ERR_INVALID_ARG, "reserved", s.reserved[4] = 1; c.depth = 17);
  PLAN(D2PC_ERR_BAD_SIZE, "2155", g.n_a = 64; g.n_b = 64; c.struct_size = 0);           // more than 2,155 cells before the terrain configuration
  PLAN(D2PC_ERR_INVALID_ARG, "terrain", c.struct_size = 28);
  PLAN(D2PC_ERR_INVALID_ARG, "terrain", c.struct_size = 0; c.depth = 99);
  PLAN(D2PC_ERR_BAD_SIZE, "depth", c.depth = 0);
  PLAN(D2PC_ERR_BAD_SIZE, "depth", c.depth = 17);
  PLAN(D2PC_ERR_BAD_SIZE, "depth", c.depth = -1);
  PLAN(D2PC_ERR_BAD_SIZE, "depth", c.depth = 17; c.reserved[3] = 1);
  for (int r = 0; r < 6; ++r) PLAN(D2PC_ERR_INVALID_ARG, "reserved", c.reserved[r] = 1);
  // ---- the sizes
  { d2pc_sectors_ground_config g = ground(5, 3); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain(3); ReliefPlan p;
    d2pc_sectors_relief_geometry_t o;
    CHECK(make_relief_plan(&g, &s, &c, &p) == D2PC_OK && 76 * 15 == 1140 && p.slot_bytes == 1152 && p.state_bytes == 256 + 3 * 1152 && p.blocks == 1);
    fill_relief_geometry(p, &o);
    CHECK(o.n_cells == 15 && o.inv_c == 2.0f && o.slot_bytes == 1152 && o.state_bytes == 3712 && o.headers_offset == 0 && o.tables_offset == 256);
    CHECK(o.blocks == 1 && o.scale == 0.0625 && o.max_tilt2 == 0.0625);
    for (int r = 0; r < 5; ++r) CHECK(o.reserved[r] == 0); }
  { d2pc_sectors_ground_config g = ground(46, 46); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain(16); ReliefPlan p;
    CHECK(make_relief_plan(&g, &s, &c, &p) == D2PC_OK && p.slot_bytes == 160816 && p.state_bytes == 256 + 16 * 160816 && p.blocks == 133); }
  { d2pc_sectors_ground_config g = ground(4, 4); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain(2); ReliefPlan p;
    CHECK(make_relief_plan(&g, &s, &c, &p) == D2PC_OK && p.slot_bytes == 1216 && p.blocks == 1);
    g = ground(6, 3); CHECK(make_relief_plan(&g, &s, &c, &p) == D2PC_OK && p.slot_bytes == 1376 && p.blocks == 2); }
  // ---- the descriptor
  DESC(D2PC_OK, (void)d);
  DESC(D2PC_OK, d.allowed = nullptr);
  { d2pc_sectors_ground_config g = ground(); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain(); ReliefPlan p;
    CHECK(make_relief_plan(&g, &s, &c, &p) == D2PC_OK && check_relief_desc(p, nullptr) == D2PC_ERR_INVALID_ARG); }
  DESC(D2PC_ERR_INVALID_ARG, d.struct_size = 152);
  DESC(D2PC_ERR_INVALID_ARG, d.struct_size = 0);
  for (int b = 0; b < 5; ++b) DESC(D2PC_ERR_INVALID_ARG, set_buf(d, b, 0));  // step and the four frame tables are required
  DESC(D2PC_ERR_INVALID_ARG, for (int o = N_IN; o < N_BUF; ++o) set_buf(d, o, 0));
  for (int only = N_IN; only < N_BUF; ++only) {
    d2pc_sectors_relief_desc d = good();
    for (int o = N_IN; o < N_BUF; ++o) if (o != only) set_buf(d, o, 0);
    expect_desc(d, D2PC_OK, __LINE__ * 100 + only);
  }
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 0);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 33);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = -1);
  DESC(D2PC_OK, d.n_candidates = 32);
  DESC(D2PC_OK, d.n_candidates = 0; d.candidates = nullptr);                // not looked at without candidates
  for (int b = 0; b < N_BUF; ++b) {
    for (size_t off = 1; off < ALIGN[b]; ++off) { d2pc_sectors_relief_desc d = good(); set_buf(d, b, BASE[b] + off); expect_desc(d, D2PC_ERR_INVALID_ARG, __LINE__ * 100 + b); }
    d2pc_sectors_relief_desc d = good(); set_buf(d, b, BASE[b] + ALIGN[b]); expect_desc(d, D2PC_OK, __LINE__ * 100 + b);
  }
  // overlaps: every output over the first and the last byte of every other buffer
  for (int o = N_IN; o < N_BUF; ++o)
    for (int b = 0; b < N_BUF; ++b) {
      if (b == o) continue;
      const size_t al = ALIGN[o], mine = SIZE[o];
      const uintptr_t first = BASE[b] - mine + al, clear_lo = BASE[b] - mine;
      const uintptr_t last = (BASE[b] + SIZE[b] - 1) / al * al, clear_hi = (BASE[b] + SIZE[b] + al - 1) / al * al;
      for (int k = 0; k < 4; ++k) {
        d2pc_sectors_relief_desc d = good();
        set_buf(d, o, k == 0 ? first : k == 1 ? clear_lo : k == 2 ? last : clear_hi);
        expect_desc(d, k % 2 == 0 ? D2PC_ERR_INVALID_ARG : D2PC_OK, __LINE__ * 10000 + o * 100 + b * 4 + k);
      }
    }
  DESC(D2PC_OK, d.allowed = nullptr; d.summary = reinterpret_cast<uint32_t *>(BASE[5] + 128));   // a buffer that is not given overlaps nothing
  DESC(D2PC_ERR_INVALID_ARG, d.count = reinterpret_cast<uint32_t *>(BASE[1]));                   // in place is refused
  DESC(D2PC_ERR_INVALID_ARG, d.moments = const_cast<int64_t *>(d.frame_moments));
  DESC(D2PC_ERR_INVALID_ARG, d.status = reinterpret_cast<uint32_t *>(BASE[4] + 7 * 2048 - 8));   // frame_moments is seven planes long
  DESC(D2PC_OK, d.status = reinterpret_cast<uint32_t *>(BASE[4] + 7 * 2048));
  // ---- the session's own state: 256 + 8 x 19,456 bytes
  { d2pc_sectors_ground_config g = ground(); d2pc_sectors_slope_config s = slope(); d2pc_sectors_terrain_config c = terrain(); ReliefPlan p;
    CHECK(make_relief_plan(&g, &s, &c, &p) == D2PC_OK && p.state_bytes == 155904);
    const d2pc_sectors_relief_desc d = good(); char msg[256] = "";
    CHECK(check_relief_state(p, &d, reinterpret_cast<const void *>(uintptr_t(0x50000000))) == D2PC_OK);
    for (int b = 0; b < N_BUF; ++b) {
      CHECK(check_relief_state(p, &d, reinterpret_cast<const void *>(BASE[b] + SIZE[b] - 1), msg, sizeof msg) == D2PC_ERR_INVALID_ARG && strstr(msg, "state"));
      CHECK(check_relief_state(p, &d, reinterpret_cast<const void *>(BASE[b] - 155904 + 1)) == D2PC_ERR_INVALID_ARG);
      CHECK(check_relief_state(p, &d, reinterpret_cast<const void *>(BASE[b] - 155904)) == D2PC_OK);
    }
    d2pc_sectors_relief_desc e = good(); e.allowed = nullptr;
    CHECK(check_relief_state(p, &e, reinterpret_cast<const void *>(BASE[5])) == D2PC_OK); }
  (void)N_OUT;
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
