// csrc/d2pc_sectors_ground_plan.hpp without a GPU and without HIP: g++ -fsanitize=address,undefined
// (tests/test_sectors_ground_cpu.py).  The refusals of a ground configuration and of a ground descriptor (the pointers are
// numbers: nothing is dereferenced), the block count as a function of max_points, the geometry and spread_of_std.
#include "d2pc_sectors_ground_plan.hpp"
#include <cmath>
using namespace d2pc::sectors;
static d2pc_sectors_ground_config config(int n_a = 16, int n_b = 16) {
  d2pc_sectors_ground_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.n_a = n_a; c.n_b = n_b; c.cell_size = 0.5f; c.quantum = 0.002f;
  c.axes[0] = 1; c.axes[1] = 2; c.axes[2] = 3; c.min_count = 4; c.max_spread_q2 = 625; c.max_step_q = 50; c.window = 1;
  c.w_dist = 1; c.w_rough = 1; c.rough_cap = 65535; return c; }
static const void *at(uintptr_t v) { return reinterpret_cast<const void *>(v); }
static void *out_at(uintptr_t v) { return reinterpret_cast<void *>(v); }
// 256 cells, 1,000 records of 16 bytes
static const uintptr_t PT = 0x20000000, CN = 0x20100000, ST = 0x20200000, AL = 0x20300000;
static const uintptr_t OUT[9] = {0x30000000, 0x30100000, 0x30200000, 0x30300000, 0x30400000, 0x30500000, 0x30600000, 0x30700000, 0x30800000};
static void set_out(d2pc_sectors_ground_desc &d, int o, uintptr_t v) {
  void *q = v ? out_at(v) : nullptr;
  switch (o) {
    case 0: d.count = static_cast<uint32_t *>(q); break;
    case 1: d.sum = static_cast<int64_t *>(q); break;
    case 2: d.sum2 = static_cast<uint64_t *>(q); break;
    case 3: d.mean_q = static_cast<int32_t *>(q); break;
    case 4: d.spread_q2 = static_cast<uint32_t *>(q); break;
    case 5: d.flat = static_cast<uint8_t *>(q); break;
    case 6: d.site = static_cast<uint8_t *>(q); break;
    case 7: d.candidates = static_cast<d2pc_sectors_ground_candidate *>(q); break;
    default: d.summary = static_cast<uint32_t *>(q); break;
  }
}
static d2pc_sectors_ground_desc good() {
  d2pc_sectors_ground_desc d; memset(&d, 0, sizeof d); d.struct_size = sizeof d; d.point_step = 16; d.n_clouds = 1; d.n_candidates = 5;
  d.points = at(PT); d.counts = static_cast<const uint32_t *>(at(CN)); d.cloud_points = 1000;
  d.step = static_cast<const d2pc_sectors_ground_step *>(at(ST)); d.allowed = static_cast<const uint8_t *>(at(AL));
  for (int o = 0; o < 9; ++o) set_out(d, o, OUT[o]);
  return d; }
static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)
static void expect_plan(const d2pc_sectors_ground_config *c, int want, int line) {
  GroundPlan p; char msg[200] = "";
  const int st = make_ground_plan(c, &p, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; return; }
  if (st == D2PC_OK && (p.n_cells != c->n_a * c->n_b || p.lds_bytes != size_t(20 * p.n_cells) || p.block_bytes < p.lds_bytes || p.block_bytes % 8 ||
                        p.block_bytes > p.lds_bytes + 4 || p.blocks_per_cu < 2 || p.blocks_per_cu > 4 || p.lds_bytes * size_t(p.blocks_per_cu) > 160u * 1024u)) {
    printf("line %d: sizes\n", line); ++fails; }
}
#define PLAN(want, ...) do { d2pc_sectors_ground_config c = config(); __VA_ARGS__; expect_plan(&c, want, __LINE__); } while (0)
static void expect_desc(const d2pc_sectors_ground_desc &d, int want, int line, int n_a = 16, int n_b = 16) {
  d2pc_sectors_ground_config c = config(n_a, n_b);
  GroundPlan p; char msg[200] = "";
  if (make_ground_plan(&c, &p) != D2PC_OK) { printf("line %d: plan\n", line); ++fails; return; }
  const int st = check_ground_desc(p, &d, msg, sizeof msg);
  if (st != want || (st != D2PC_OK && !msg[0])) { printf("line %d: status %d, not %d (%s)\n", line, st, want, msg); ++fails; }
}
#define DESC(want, ...) do { d2pc_sectors_ground_desc d = good(); __VA_ARGS__; expect_desc(d, want, __LINE__); } while (0)
int main() {
  // ---- the configuration: every INVALID_ARG before the first BAD_SIZE
  PLAN(D2PC_OK, (void)c);
  PLAN(D2PC_OK, c.n_a = 2; c.n_b = 64; c.window = 8; c.w_dist = c.w_rough = 4095; c.rough_cap = c.max_step_q = 65535; c.max_spread_q2 = 0xFFFFFFFFu);
  PLAN(D2PC_OK, c.n_a = 64; c.n_b = 64; c.window = 0; c.w_dist = c.w_rough = 0; c.rough_cap = c.max_step_q = 0; c.max_spread_q2 = 0; c.max_points = 0xFFFFFFFFu);
  PLAN(D2PC_OK, c.n_a = 5; c.n_b = 3; c.axes[0] = -2; c.axes[1] = 1; c.axes[2] = -3);
  expect_plan(nullptr, D2PC_ERR_INVALID_ARG, __LINE__);
  PLAN(D2PC_ERR_INVALID_ARG, c.struct_size = 76);
  PLAN(D2PC_ERR_INVALID_ARG, c.axes[1] = 1);
  PLAN(D2PC_ERR_INVALID_ARG, c.axes[2] = 4);
  PLAN(D2PC_ERR_INVALID_ARG, c.axes[0] = 0);
  PLAN(D2PC_ERR_INVALID_ARG, c.axes[0] = INT32_MIN);
  PLAN(D2PC_ERR_INVALID_ARG, c.cell_size = 0.f);
  PLAN(D2PC_ERR_INVALID_ARG, c.cell_size = -0.5f);
  PLAN(D2PC_ERR_INVALID_ARG, c.cell_size = NAN);
  PLAN(D2PC_ERR_INVALID_ARG, c.cell_size = INFINITY);
  PLAN(D2PC_ERR_INVALID_ARG, c.quantum = 0.f);
  PLAN(D2PC_ERR_INVALID_ARG, c.quantum = -1.f);
  PLAN(D2PC_ERR_INVALID_ARG, c.quantum = NAN);
  PLAN(D2PC_ERR_INVALID_ARG, c.quantum = INFINITY);
  PLAN(D2PC_ERR_INVALID_ARG, c.min_count = 0);
  PLAN(D2PC_ERR_INVALID_ARG, c.max_step_q = 65536);
  PLAN(D2PC_ERR_INVALID_ARG, c.w_dist = 4096);
  PLAN(D2PC_ERR_INVALID_ARG, c.w_rough = 4096);
  PLAN(D2PC_ERR_INVALID_ARG, c.rough_cap = 65536);
  PLAN(D2PC_ERR_INVALID_ARG, c.reserved[0] = 1);
  PLAN(D2PC_ERR_INVALID_ARG, c.reserved[2] = 1);
  PLAN(D2PC_ERR_INVALID_ARG, c.quantum = 0.f; c.n_a = 99);                  // INVALID_ARG before BAD_SIZE
  PLAN(D2PC_ERR_BAD_SIZE, c.n_a = 1);
  PLAN(D2PC_ERR_BAD_SIZE, c.n_a = 65);
  PLAN(D2PC_ERR_BAD_SIZE, c.n_b = 1);
  PLAN(D2PC_ERR_BAD_SIZE, c.n_b = 65);
  PLAN(D2PC_ERR_BAD_SIZE, c.n_b = -4);
  PLAN(D2PC_ERR_BAD_SIZE, c.window = -1);
  PLAN(D2PC_ERR_BAD_SIZE, c.window = 9);
  PLAN(D2PC_ERR_BAD_SIZE, c.cell_size = 1e-45f);                            // 1 / cell_size is +inf in float32
  PLAN(D2PC_ERR_BAD_SIZE, c.quantum = 2e-39f);
  PLAN(D2PC_OK, c.cell_size = 3e38f);                                       // a denormal inverse is positive and finite
  // ---- the blocks: one per four shares of max_points, 1 .. blocks_per_cu x compute units
  CHECK(ground_blocks(0, 4, 256) == 1024 && ground_blocks(0, 2, 256) == 512 && ground_blocks(0, 4, 0) == 4);
  CHECK(ground_blocks(1, 4, 256) == 1 && ground_blocks(1024, 4, 256) == 1 && ground_blocks(1025, 4, 256) == 1);
  CHECK(ground_blocks(4096, 4, 256) == 1 && ground_blocks(4097, 4, 256) == 2);
  CHECK(ground_blocks(3000000, 4, 256) == 733 && ground_blocks(3000000, 2, 256) == 512);
  CHECK(ground_blocks(0xFFFFFFFFu, 4, 256) == 1024 && ground_blocks(0xFFFFFFFFu, 2, 256) == 512 && ground_blocks(0xFFFFFFFFu, 4, 1) == 4);
  { d2pc_sectors_ground_config c = config(64, 64); c.max_points = 360960; GroundPlan p; d2pc_sectors_ground_geometry_t g;
    CHECK(make_ground_plan(&c, &p) == D2PC_OK); fill_ground_geometry(p, &g);
    CHECK(g.n_cells == 4096 && g.lds_bytes == 81920 && g.block_bytes == 81920 && g.blocks_per_cu == 2 && g.blocks == 89 && g.share_points == 1024);
    CHECK(g.device_bytes == 89u * 81920u + 13u * 4096u && g.inv_c == 2.0f && g.inv_q == float(1.0 / double(0.002f))); }
  { d2pc_sectors_ground_config c = config(5, 3); GroundPlan p; CHECK(make_ground_plan(&c, &p) == D2PC_OK && p.lds_bytes == 300 && p.block_bytes == 304); }
  // ---- spread_of_std
  CHECK(ground_spread_of_std(0.002, 0.05) == 625 && ground_spread_of_std(1.0, 0.0) == 0 && ground_spread_of_std(1.0, 2.5) == 6);
  CHECK(ground_spread_of_std(1.0, 65535.9) == uint32_t(std::floor(65535.9 * 65535.9)) && ground_spread_of_std(1.0, 65536.0) == 0xFFFFFFFEu);
  CHECK(ground_spread_of_std(1e-9, 1e9) == 0xFFFFFFFEu && ground_spread_of_std(1.0, INFINITY) == 0xFFFFFFFEu);
  CHECK(ground_spread_of_std(0.0, 1.0) == 0 && ground_spread_of_std(-1.0, 1.0) == 0 && ground_spread_of_std(NAN, 1.0) == 0 &&
        ground_spread_of_std(1.0, NAN) == 0 && ground_spread_of_std(1.0, -0.5) == 0 && ground_spread_of_std(INFINITY, 1.0) == 0);
  // ---- the descriptor
  DESC(D2PC_OK, (void)d);
  DESC(D2PC_OK, d.counts = nullptr; d.allowed = nullptr);
  DESC(D2PC_OK, d.point_step = 32);
  expect_desc(good(), D2PC_OK, __LINE__, 64, 64);
  DESC(D2PC_ERR_INVALID_ARG, d.struct_size = 128);
  DESC(D2PC_ERR_INVALID_ARG, d.point_step = 12);
  DESC(D2PC_ERR_INVALID_ARG, d.n_clouds = 0);
  DESC(D2PC_ERR_INVALID_ARG, d.n_clouds = 65536);
  DESC(D2PC_ERR_INVALID_ARG, d.points = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, d.step = nullptr);
  DESC(D2PC_ERR_INVALID_ARG, for (int o = 0; o < 9; ++o) set_out(d, o, 0));
  for (int only = 0; only < 9; ++only) {
    d2pc_sectors_ground_desc d = good();
    for (int o = 0; o < 9; ++o) if (o != only) set_out(d, o, 0);
    expect_desc(d, D2PC_OK, __LINE__ * 100 + only);
  }
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 0);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 33);
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = -1);
  DESC(D2PC_OK, d.n_candidates = 32);
  DESC(D2PC_OK, d.n_candidates = 0; d.candidates = nullptr);                // not looked at without candidates
  DESC(D2PC_ERR_INVALID_ARG, d.points = at(PT + 8));
  DESC(D2PC_ERR_INVALID_ARG, d.counts = static_cast<const uint32_t *>(at(CN + 2)));
  DESC(D2PC_ERR_INVALID_ARG, d.step = static_cast<const d2pc_sectors_ground_step *>(at(ST + 2)));
  DESC(D2PC_OK, d.step = static_cast<const d2pc_sectors_ground_step *>(at(ST + 4)); d.allowed = static_cast<const uint8_t *>(at(AL + 1)));
  { const size_t align[9] = {4, 8, 8, 4, 4, 1, 1, 8, 4};
    for (int o = 0; o < 9; ++o) {
      for (size_t off = 1; off < align[o]; ++off) { d2pc_sectors_ground_desc d = good(); set_out(d, o, OUT[o] + off); expect_desc(d, D2PC_ERR_INVALID_ARG, __LINE__ * 100 + o); }
      d2pc_sectors_ground_desc d = good(); set_out(d, o, OUT[o] + align[o]); expect_desc(d, D2PC_OK, __LINE__ * 100 + o);
    } }
  // the cloud sizes: BAD_SIZE, after every INVALID_ARG but the overlaps
  DESC(D2PC_ERR_BAD_SIZE, d.cloud_points = 0);
  DESC(D2PC_ERR_BAD_SIZE, d.cloud_points = size_t(1) << 32);
  DESC(D2PC_ERR_BAD_SIZE, d.n_clouds = 2; d.points_frame_stride_points = 999);
  DESC(D2PC_ERR_BAD_SIZE, d.n_clouds = 3; d.points_frame_stride_points = size_t(1) << 31);
  DESC(D2PC_ERR_INVALID_ARG, d.cloud_points = 0; d.step = nullptr);
  DESC(D2PC_OK, d.n_clouds = 3; d.points_frame_stride_points = 1000);
  // overlaps: every output over the first and the last byte of every other buffer
  { const uintptr_t base[13] = {PT, CN, ST, AL, OUT[0], OUT[1], OUT[2], OUT[3], OUT[4], OUT[5], OUT[6], OUT[7], OUT[8]};
    const size_t size[13] = {16000, 4, 80, 256, 1024, 2048, 2048, 1024, 1024, 256, 256, 40, 16};
    const size_t align[9] = {4, 8, 8, 4, 4, 1, 1, 8, 4};
    for (int o = 0; o < 9; ++o)
      for (int b = 0; b < 13; ++b) {
        if (b == o + 4) continue;
        const size_t al = align[o], mine = size[o + 4];
        const uintptr_t first = base[b] - mine + al, clear_lo = base[b] - mine;
        const uintptr_t last = (base[b] + size[b] - 1) / al * al, clear_hi = (base[b] + size[b] + al - 1) / al * al;
        for (int k = 0; k < 4; ++k) {
          d2pc_sectors_ground_desc d = good();
          set_out(d, o, k == 0 ? first : k == 1 ? clear_lo : k == 2 ? last : clear_hi);
          expect_desc(d, k % 2 == 0 ? D2PC_ERR_INVALID_ARG : D2PC_OK, __LINE__ * 10000 + o * 100 + b * 4 + k);
        }
      }
  }
  DESC(D2PC_OK, d.allowed = nullptr; d.summary = static_cast<uint32_t *>(out_at(AL + 128)));     // a buffer that is not given overlaps nothing
  DESC(D2PC_OK, d.n_candidates = 1; d.summary = static_cast<uint32_t *>(out_at(OUT[7] + 8)));     // the candidates' extent is n_candidates
  DESC(D2PC_ERR_INVALID_ARG, d.n_candidates = 2; d.summary = static_cast<uint32_t *>(out_at(OUT[7] + 8)));
  DESC(D2PC_ERR_INVALID_ARG, d.n_clouds = 3; d.points_frame_stride_points = 5000; d.summary = static_cast<uint32_t *>(out_at(PT + 16 * 10999)));
  DESC(D2PC_OK, d.n_clouds = 3; d.points_frame_stride_points = 5000; d.summary = static_cast<uint32_t *>(out_at(PT + 16 * 11000)));
  // the extents follow the session's cells: 4,096
  { d2pc_sectors_ground_desc d = good(); d.summary = static_cast<uint32_t *>(out_at(OUT[1] + 8 * 4096 - 8)); expect_desc(d, D2PC_ERR_INVALID_ARG, __LINE__, 64, 64);
    d.summary = static_cast<uint32_t *>(out_at(OUT[1] + 8 * 4096)); expect_desc(d, D2PC_OK, __LINE__, 64, 64);
    d.summary = static_cast<uint32_t *>(out_at(AL + 4092)); expect_desc(d, D2PC_ERR_INVALID_ARG, __LINE__, 64, 64);
    d.summary = static_cast<uint32_t *>(out_at(AL + 4096)); expect_desc(d, D2PC_OK, __LINE__, 64, 64); }
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
