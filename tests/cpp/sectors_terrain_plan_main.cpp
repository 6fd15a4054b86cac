// csrc/d2pc_sectors_terrain_plan.hpp without a GPU and without the device runtime: g++ -fsanitize=address,undefined
// (tests/test_sectors_terrain_cpu.py).  The refusals of a terrain configuration (the ground configuration's first), the
// sizes of the state block, and the refusals of a terrain descriptor, the overlap with the session's state included (the
// pointers are numbers: nothing is dereferenced).
#include "d2pc_sectors_terrain_plan.hpp"
using namespace d2pc::sectors;
static d2pc_sectors_ground_config ground(int n_a = 16, int n_b = 16) {
  d2pc_sectors_ground_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.n_a = n_a; c.n_b = n_b; c.cell_size = 0.5f; c.quantum = 0.002f;
  c.axes[0] = 1; c.axes[1] = 2; c.axes[2] = 3; c.min_count = 4; c.max_spread_q2 = 625; c.max_step_q = 50; c.window = 1;
  c.w_dist = 1; c.w_rough = 1; c.rough_cap = 65535; return c; }
static d2pc_sectors_terrain_config terrain(int depth = 8) {
  d2pc_sectors_terrain_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.depth = depth; return c; }
// 256 cells: the five inputs, then the ten outputs
static const int N_IN = 5, N_OUT = 10, N_BUF = 15;
static const uintptr_t BASE[N_BUF] = {0x20000000, 0x20100000, 0x20200000, 0x20300000, 0x20400000, 0x30000000, 0x30100000, 0x30200000,
                                      0x30300000, 0x30400000, 0x30500000, 0x30600000, 0x30700000, 0x30800000, 0x30900000};
static const size_t SIZE[N_BUF] = {80, 1024, 2048, 2048, 256, 1024, 2048, 2048, 1024, 1024, 256, 256, 40, 16, 16};
static const size_t ALIGN[N_BUF] = {4, 4, 8, 8, 1, 4, 8, 8, 4, 4, 1, 1, 8, 4, 4};
static void set_buf(d2pc_sectors_terrain_desc &d, int b, uintptr_t v) {
  void *q = v ? reinterpret_cast<void *>(v) : nullptr;
  switch (b) {
    case 0: d.step = static_cast<const d2pc_sectors_ground_step *>(q); break;
    case 1: d.frame_count = static_cast<const uint32_t *>(q); break;
    case 2: d.frame_sum = static_cast<const int64_t *>(q); break;
    case 3: d.frame_sum2 = static_cast<const uint64_t *>(q); break;
    case 4: d.allowed = static_cast<const uint8_t *>(q); break;
    case 5: d.count = static_cast<uint32_t *>(q); break;
    case 6: d.sum = static_cast<int64_t *>(q); break;
    case 7: d.sum2 = static_cast<uint64_t *>(q); break;
    case 8: d.mean_q = static_cast<int32_t *>(q); break;
    case 9: d.spread_q2 = static_cast<uint32_t *>(q); break;
    case 10: d.flat = static_cast<uint8_t *>(q); break;
    case 11: d.site = static_cast<uint8_t *>(q); break;
    case 12: d.candidates = static_cast<d2pc_sectors_ground_candidate *>(q); break;
    case 13: d.summary = static_cast<uint32_t *>(q); break;
    default: d.status = static_cast<uint32_t *>(q); break;
  }
}
static d2pc_sectors_terrain_desc good() {
  d2pc_sectors_terrain_desc d; memset(&d, 0, sizeof d); d.struct_size = sizeof d; d.n_candidates = 5;
  for (int b = 0; b < N_BUF; ++b) set_buf(d, b, BASE[b]);
  return d; }
static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)
static void expect_plan(const d2pc_sectors_ground_config *g, const d2pc_sectors_terrain_config *c, int want, int line) {
  TerrainPlan p; char msg[200] = "";
  const int st = make_terrain_plan(g, c, &p, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; return; }
  if (st == D2PC_OK && (p.depth != c->depth || p.slot_bytes % 16 || p.slot_bytes < size_t(20 * p.ground.n_cells) || p.slot_bytes >= size_t(20 * p.ground.n_cells) + 16 ||
                        p.state_bytes != 256 + size_t(p.depth) * p.slot_bytes)) { printf("line %d: sizes\n", line); ++fails; }
}
#define PLAN(want, ...) do { d2pc_sectors_ground_config g = ground(); d2pc_sectors_terrain_config c = terrain(); __VA_ARGS__; expect_plan(&g, &c, want, __LINE__); } while (0)
static void expect_desc(const d2pc_sectors_terrain_desc &d, int want, int line, int n_a = 16, int n_b = 16) {
  d2pc_sectors_ground_config g = ground(n_a, n_b); d2pc_sectors_terrain_config c = terrain();
  TerrainPlan p; char msg[200] = "";
  if (make_terrain_plan(&g, &c, &p) != D2PC_OK) { printf("line %d: plan\n", line); ++fails; return; }
  const int st = check_terrain_desc(p, &d, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; }
}
#define DESC(want, ...) do { d2pc_sectors_terrain_desc d = good(); __VA_ARGS__; expect_desc(d, want, __LINE__); } while (0)
int main() {
  // ---- the configurations: the ground's refusals first and unchanged
  PLAN(D2PC_OK, (void)c);
  PLAN(D2PC_OK, c.depth = 1);
  PLAN(D2PC_OK, c.depth = 16; g.n_a = 64; g.n_b = 64);
  PLAN(D2PC_OK, c.depth = 3; g.n_a = 5; g.n_b = 3);
  { d2pc_sectors_ground_config g = ground(); d2pc_sectors_terrain_config c = terrain();
    expect_plan(nullptr, &c, D2PC_ERR_INVALID_ARG, __LINE__); expect_plan(&g, nullptr, D2PC_ERR_INVALID_ARG, __LINE__); }
  PLAN(D2PC_ERR_INVALID_ARG, g.struct_size = 76);
  PLAN(D2PC_ERR_INVALID_ARG, g.quantum = 0.f; c.depth = 0);
  PLAN(D2PC_ERR_BAD_SIZE, g.n_a = 65; c.struct_size = 0);                     // the ground's BAD_SIZE before the terrain's INVALID_ARG
  PLAN(D2PC_ERR_BAD_SIZE, g.window = 9; c.reserved[0] = 1);
  PLAN(D2PC_ERR_INVALID_ARG, c.struct_size = 28);
  PLAN(D2PC_ERR_INVALID_ARG, c.struct_size = 0);
  PLAN(D2PC_ERR_INVALID_ARG, c.struct_size = 0; c.depth = 99);
  PLAN(D2PC_ERR_BAD_SIZE, c.depth = 0);
  PLAN(D2PC_ERR_BAD_SIZE, c.depth = 17);
  PLAN(D2PC_ERR_BAD_SIZE, c.depth = -1);
  PLAN(D2PC_ERR_BAD_SIZE, c.depth = 17; c.reserved[3] = 1);                   // in the order the header lists them
  for (int r = 0; r < 6; ++r) PLAN(D2PC_ERR_INVALID_ARG, c.reserved[r] = 1);
  // ---- the sizes
  { d2pc_sectors_ground_config g = ground(5, 3); d2pc_sectors_terrain_config c = terrain(3); TerrainPlan p; d2pc_sectors_terrain_geometry_t o;
    CHECK(make_terrain_plan(&g, &c, &p) == D2PC_OK && p.slot_bytes == 304 && p.state_bytes == 256 + 3 * 304); fill_terrain_geometry(p, &o);
    CHECK(o.n_cells == 15 && o.inv_c == 2.0f && o.slot_bytes == 304 && o.state_bytes == 1168 && o.headers_offset == 0 && o.tables_offset == 256); }
  { d2pc_sectors_ground_config g = ground(64, 64); d2pc_sectors_terrain_config c = terrain(16); TerrainPlan p;
    CHECK(make_terrain_plan(&g, &c, &p) == D2PC_OK && p.slot_bytes == 81920 && p.state_bytes == 256 + 16 * 81920); }
  { d2pc_sectors_ground_config g = ground(33, 31); d2pc_sectors_terrain_config c = terrain(2); TerrainPlan p;
    CHECK(make_terrain_plan(&g, &c, &p) == D2PC_OK && p.slot_bytes == 20464 && 20 * 1023 == 20460); }
  // ---- the descriptor
  DESC(D2PC_OK, (void)d);
  DESC(D2PC_OK, d.allowed = nullptr);
  expect_desc(good(), D2PC_OK, __LINE__, 64, 64);
  { d2pc_sectors_ground_config g = ground(); d2pc_sectors_terrain_config c = terrain(); TerrainPlan p;
    CHECK(make_terrain_plan(&g, &c, &p) == D2PC_OK && check_terrain_desc(p, nullptr) == D2PC_ERR_INVALID_ARG); }
  DESC(D2PC_ERR_INVALID_ARG, d.struct_size = 120);
  DESC(D2PC_ERR_INVALID_ARG, d.struct_size = 0);
  for (int b = 0; b < 4; ++b) DESC(D2PC_ERR_INVALID_ARG, set_buf(d, b, 0));  // step and the three frame tables are required
  DESC(D2PC_ERR_INVALID_ARG, for (int o = N_IN; o < N_BUF; ++o) set_buf(d, o, 0));
  for (int only = N_IN; only < N_BUF; ++only) {
    d2pc_sectors_terrain_desc d = good();
    for (int o = N_IN; o < N_BUF; ++o) if (o != only) set_buf(d, o, 0);
    expect_desc(d, D2PC_OK, __LINE__ * 100 + only);
  }
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 0);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 33);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = -1);
  DESC(D2PC_OK, d.n_candidates = 32);
  DESC(D2PC_OK, d.n_candidates = 0; d.candidates = nullptr);                // not looked at without candidates
  for (int b = 0; b < N_BUF; ++b) {
    for (size_t off = 1; off < ALIGN[b]; ++off) { d2pc_sectors_terrain_desc d = good(); set_buf(d, b, BASE[b] + off); expect_desc(d, D2PC_ERR_INVALID_ARG, __LINE__ * 100 + b); }
    d2pc_sectors_terrain_desc d = good(); set_buf(d, b, BASE[b] + ALIGN[b]); expect_desc(d, D2PC_OK, __LINE__ * 100 + b);
  }
  // overlaps: every output over the first and the last byte of every other buffer
  for (int o = N_IN; o < N_BUF; ++o)
    for (int b = 0; b < N_BUF; ++b) {
      if (b == o) continue;
      const size_t al = ALIGN[o], mine = SIZE[o];
      const uintptr_t first = BASE[b] - mine + al, clear_lo = BASE[b] - mine;
      const uintptr_t last = (BASE[b] + SIZE[b] - 1) / al * al, clear_hi = (BASE[b] + SIZE[b] + al - 1) / al * al;
      for (int k = 0; k < 4; ++k) {
        d2pc_sectors_terrain_desc d = good();
        set_buf(d, o, k == 0 ? first : k == 1 ? clear_lo : k == 2 ? last : clear_hi);
        expect_desc(d, k % 2 == 0 ? D2PC_ERR_INVALID_ARG : D2PC_OK, __LINE__ * 10000 + o * 100 + b * 4 + k);
      }
    }
  DESC(D2PC_OK, d.allowed = nullptr; d.summary = reinterpret_cast<uint32_t *>(BASE[4] + 128));   // a buffer that is not given overlaps nothing
  DESC(D2PC_OK, d.n_candidates = 1; d.summary = reinterpret_cast<uint32_t *>(BASE[12] + 8));     // the candidates' extent is n_candidates
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 2; d.summary = reinterpret_cast<uint32_t *>(BASE[12] + 8));
  DESC(D2PC_OK, d.count = reinterpret_cast<uint32_t *>(BASE[1] + 1024));                         // inputs may not be outputs, neighbours may
  DESC(D2PC_ERR_INVALID_ARG, d.count = reinterpret_cast<uint32_t *>(BASE[1]));                   // in place is refused
  // the extents follow the session's cells: 4,096
  { d2pc_sectors_terrain_desc d = good(); d.status = reinterpret_cast<uint32_t *>(BASE[2] + 8 * 4096 - 8); expect_desc(d, D2PC_ERR_INVALID_ARG, __LINE__, 64, 64);
    d.status = reinterpret_cast<uint32_t *>(BASE[2] + 8 * 4096); expect_desc(d, D2PC_OK, __LINE__, 64, 64); }
  // ---- the session's own state: 256 + 8 x 5,120 bytes
  { d2pc_sectors_ground_config g = ground(); d2pc_sectors_terrain_config c = terrain(); TerrainPlan p;
    CHECK(make_terrain_plan(&g, &c, &p) == D2PC_OK && p.state_bytes == 41216);
    const d2pc_sectors_terrain_desc d = good(); char msg[200] = "";
    CHECK(check_terrain_state(p, &d, reinterpret_cast<const void *>(uintptr_t(0x50000000))) == D2PC_OK);
    for (int b = 0; b < N_BUF; ++b) {
      CHECK(check_terrain_state(p, &d, reinterpret_cast<const void *>(BASE[b] + SIZE[b] - 1), msg, sizeof msg) == D2PC_ERR_INVALID_ARG && msg[0]);
      CHECK(check_terrain_state(p, &d, reinterpret_cast<const void *>(BASE[b] - 41216 + 1)) == D2PC_ERR_INVALID_ARG);
      CHECK(check_terrain_state(p, &d, reinterpret_cast<const void *>(BASE[b] - 41216)) == D2PC_OK);
    }
    d2pc_sectors_terrain_desc e = good(); e.allowed = nullptr;
    CHECK(check_terrain_state(p, &e, reinterpret_cast<const void *>(BASE[4])) == D2PC_OK); }
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
