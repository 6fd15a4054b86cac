// csrc/d2pc_route.hpp without a GPU and without HIP: g++ -fsanitize=address,undefined (tests/test_route_plan_cpu.py).
//   route_plan          reads one query per line on stdin and prints one line of plan per query (the test compares them
//                       with tests/route_model.py)
//   route_plan check    enumerates a grid of its own and checks what a plan must satisfy whatever the thresholds are;
//                       exits non-zero on the first failure
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../disparity_to_point_cloud_amd/csrc/d2pc_route.hpp"

using namespace d2pc;
using namespace d2pc::host;

namespace {

RouteTuning product_tuning(int cu) {
  RouteTuning t{};
  t.cu_count = cu;
  t.blocks_per_cu = 128;
  t.resident_stagger_pct = -1;
  t.big_batch_algo = 2;
  t.chunk_mb = 96;
  return t;
}

// ---- queries ----------------------------------------------------------------------------------------------------------
//   C cu compact_algo force_algo resident_pxt onepass_form captured n_frames roi_n pxt elem_size is_f32
//     -> C split algo pxt form grid stagger_on self_clean
//   B cu per_cu fused_form tiles_x tiles_y n_frames
//     -> B resident nfc sub_batches | per_frame grid pipelined (a full sub-batch) | ns per_frame grid pipelined (the last)
//   O cb_chunks cb_fused cb_fused_compact width height n_frames median bridge16 captured compact bs_median roi_w
//     -> O overlap chunk one_kernel
//   P pxt_parity is_f32 border width height n_frames
//     -> P pxt
int answer_queries() {
  char line[256];
  long n_lines = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    ++n_lines;
    long long v[12] = {0};
    const int got = std::sscanf(line + 1, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4,
                                v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11);
    if (line[0] == 'C' && got == 11) {
      RouteTuning t = product_tuning(int(v[0]));
      t.compact_algo = int(v[1]);
      t.resident_pxt = int(v[3]);
      t.onepass_form = int(v[4]);
      CompactCall c{};
      c.force_algo = int(v[2]);
      c.captured = v[5] != 0;
      c.n_frames = uint32_t(v[6]);
      c.roi_n = uint32_t(v[7]);
      c.pxt = int(v[8]);
      c.elem_size = int(v[9]);
      c.is_f32 = v[10] != 0;
      const CompactPlan p = plan_compact(t, c);
      std::printf("C %d %d %d %d %u %d %d\n", int(p.split), p.algo, p.pxt, p.onepass_form, p.grid, int(p.stagger != 0), int(p.self_clean));
    } else if (line[0] == 'B' && got == 6) {
      const uint32_t n = uint32_t(v[5]);
      const CallbackCompactPlan p = plan_callback_compact(int(v[0]), int(v[1]), int(v[2]), uint32_t(v[3]), uint32_t(v[4]), n);
      const uint32_t full = n < p.nfc ? n : p.nfc, last = n - (p.sub_batches - 1) * p.nfc;
      const CallbackCompactPlan::Sub a = p.sub(full), b = p.sub(last);
      std::printf("B %u %u %u | %u %u %d | %u %u %u %d\n", p.resident, p.nfc, p.sub_batches, a.per_frame, a.grid, int(a.pipelined), last,
                  b.per_frame, b.grid, int(b.pipelined));
    } else if (line[0] == 'O' && got == 12) {
      const CallbackTuning t{int(v[0]), int(v[1]), int(v[2])};
      CallbackCall c{};
      c.width = int(v[3]);
      c.height = int(v[4]);
      c.n_frames = int(v[5]);
      c.median = v[6] != 0;
      c.bridge16 = v[7] != 0;
      c.captured = v[8] != 0;
      c.compact = v[9] != 0;
      c.bs_median = v[10] != 0;
      c.roi_w = uint32_t(v[11]);
      const CallbackPlan p = plan_callback(t, c);
      std::printf("O %d %d %d\n", int(p.overlap), p.chunk, int(p.one_kernel));
    } else if (line[0] == 'P' && got == 6) {
      std::printf("P %d\n", parity_pxt(int(v[0]), v[1] != 0, int(v[2]), int(v[3]), int(v[4]), int(v[5])));
    } else {
      std::printf("BAD QUERY in line %ld: %s", n_lines, line);
      return 2;
    }
  }
  return 0;
}

// ---- invariants -------------------------------------------------------------------------------------------------------
[[noreturn]] void die(const char *what, const RouteTuning &t, const CompactCall &c, const CompactPlan &p) {
  std::printf("FAILED %s: cu %d, compact_algo %d, resident_pxt %d, unbounded %d, onepass_form %d, onepass_blocks_per_cu %d | roi_n %u, "
              "frames %u, pxt %d, captured %d, force %d -> split %d, algo %d, pxt %d, grid %u\n",
              what, t.cu_count, t.compact_algo, t.resident_pxt, t.resident_unbounded, t.onepass_form, t.onepass_blocks_per_cu, c.roi_n,
              c.n_frames, c.pxt, int(c.captured), c.force_algo, int(p.split), p.algo, p.pxt, p.grid);
  std::exit(1);
}

long check_compact_plan(const RouteTuning &t, const CompactCall &c) {
  const CompactPlan p = plan_compact(t, c);
  const uint32_t cap = uint32_t(t.cu_count) * uint32_t(kResidentBlocksPerCu);
  if (p.split) {
    if (c.n_frames != 2 || c.captured || c.force_algo || (t.compact_algo != 0 && t.compact_algo != 3)) die("split of such a call", t, c, p);
    CompactCall one = c;
    one.n_frames = 1;
    const CompactPlan q = plan_compact(t, one);  // what each of the two launches gets
    if (q.split || q.algo != 3) die("split, and a single frame is not resident-routable", t, c, p);
    return 1;
  }
  if (p.grid < 1) die("empty grid", t, c, p);
  if (p.algo < 1 || p.algo > 4) die("no algorithm", t, c, p);
  if (p.algo == 1 && p.pxt != c.pxt) die("the two-pass form outside the caller's tiles", t, c, p);
  if (p.algo == 2 && p.grid < c.n_frames) die("single pass with fewer blocks than frames", t, c, p);
  if (p.self_clean && p.algo != 2) die("self-cleaning launch that is no single pass", t, c, p);
  if (p.algo == 3) {
    const uint64_t tpf = (uint64_t(c.roi_n) + uint64_t(256 * p.pxt) - 1) / uint64_t(256 * p.pxt);
    if (c.captured) die("resident blocks in a capture", t, c, p);
    if (p.grid != tpf * c.n_frames) die("resident grid is not one block per tile", t, c, p);
    if (!t.resident_unbounded && (tpf * c.n_frames > cap || tpf > 1024)) die("resident blocks that do not fit", t, c, p);
    if (p.lean != (p.pxt != c.pxt) || (!p.lean && p.stagger)) die("ramp outside the register-resident form", t, c, p);
  } else if (p.stagger || p.lean) {
    die("ramp without resident blocks", t, c, p);
  }
  return 1;
}

long check_compact() {
  long plans = 0;
  for (int cu : {8, 64, 104, 256, 304}) {
    const uint32_t cap = uint32_t(cu * kResidentBlocksPerCu);
    for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 16u, cap + 1u, 65535u})
      for (int algo = 0; algo <= 4; ++algo)
        for (int force = 0; force <= 4; ++force)
          for (int rpxt : {0, 8, 32, 64})
            for (int unbounded = 0; unbounded <= 1; ++unbounded)
              for (int form : {0, 1, 2, 3, 4})
                for (int per_cu : {0, 1})
                  for (int captured = 0; captured <= 1; ++captured)
                    for (int pxt : {4, 8})
                      for (int r : {pxt, 32, 64})
                        for (uint32_t k : {1u, cap / n, cap / n + 1u, 1024u, 1025u, 5120u})
                          for (int d = -1; d <= 1; ++d) {
                            const long long roi_n = 256ll * r * k + d;
                            if (roi_n < 1 || roi_n > (1ll << 28)) continue;
                            if ((roi_n + 256 * pxt - 1) / (256 * pxt) * n > 0x7fffffffll) continue;  // (make_geom refuses the batch)
                            RouteTuning t = product_tuning(cu);
                            t.compact_algo = algo;
                            t.resident_pxt = rpxt;
                            t.resident_unbounded = unbounded;
                            t.onepass_form = form;
                            t.onepass_blocks_per_cu = per_cu;
                            t.big_batch_algo = (algo + force) % 2 ? 4 : 2;
                            CompactCall c{};
                            c.roi_n = uint32_t(roi_n);
                            c.n_frames = n;
                            c.pxt = pxt;
                            c.elem_size = d == 0 ? 1 : 4;
                            c.is_f32 = d != 0;
                            c.captured = captured != 0;
                            c.force_algo = force;
                            plans += check_compact_plan(t, c);
                          }
  }
  return plans;
}

long check_callback() {
  long plans = 0;
  for (int cu : {8, 42, 43, 64, 256, 304})
    for (int per_cu = 1; per_cu <= 4; ++per_cu)
      for (int form = 1; form <= 2; ++form)
        for (uint32_t tiles_x : {1u, 2u, 3u, 5u, 16u, 17u, 127u, 128u})
          for (uint32_t tiles_y : {1u, 2u, 3u, 130u}) {
            const uint32_t resident = uint32_t(cu) * uint32_t(per_cu < 3 ? per_cu : 3);
            const uint32_t nfc0 = resident / (tiles_x + 1u);
            const uint32_t top = 2u * (nfc0 ? nfc0 : 1u) + 2u;
            for (uint32_t n = 1; n <= top; ++n) {
              const CallbackCompactPlan p = plan_callback_compact(cu, per_cu, form, tiles_x, tiles_y, n);
              auto fail = [&](const char *what) {
                std::printf("FAILED callback %s: cu %d, per_cu %d, form %d, tiles %u x %u, frames %u -> resident %u, nfc %u\n", what, cu,
                            per_cu, form, tiles_x, tiles_y, n, p.resident, p.nfc);
                std::exit(1);
              };
              if (p.resident != resident || p.nfc < 1 || p.tpf != tiles_x * tiles_y) fail("residency");
              uint32_t covered = 0, subs = 0;
              for (uint32_t s0 = 0; s0 < n; s0 += p.nfc, ++subs) {  // the caller's loop
                const uint32_t ns = n - s0 < p.nfc ? n - s0 : p.nfc;
                covered += ns;
                const CallbackCompactPlan::Sub s = p.sub(ns);
                if (s.grid != s.per_frame * ns || s.grid < ns) fail("grid is not per_frame x frames");
                if (s.pipelined) {
                  if (form != 2) fail("pipelined form that was not asked for");
                  if (!(s.per_frame > tiles_x || s.per_frame == p.tpf)) fail("pipelined with no more blocks than a band has tiles");
                  if (s.per_frame > p.tpf || s.grid > resident) fail("more persistent blocks than tiles or than are resident");
                } else {
                  if (s.per_frame != p.tpf) fail("one tile per block with another grid");
                  if (nfc0 >= 1 && uint64_t(ns) * tiles_x > uint64_t(resident) - ns) fail("a band of blocks per frame is not resident");
                }
              }
              if (covered != n || subs != p.sub_batches) fail("the sub-batches do not cover every frame once");
              ++plans;
            }
          }
  return plans;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "check")) {
    const long compact = check_compact(), callback = check_callback();
    std::printf("route check ok: %ld compact plans, %ld callback plans\n", compact, callback);
    return 0;
  }
  return answer_queries();
}
