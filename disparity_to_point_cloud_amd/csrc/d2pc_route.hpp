// d2pc_route.hpp -- which kernel serves a call, in which tile shape and grid: the launch plans of a COMPACT call
// (plan_compact, for enqueue) and of the callback body (plan_callback, plan_callback_compact, for
// d2pc_process_mono_device), and the constants they interpret.  Pure functions of numbers and small structs: no context,
// no device pointer, no allocation.  Host code only and no HIP: plain g++ compiles it (tests/cpp/route_plan_main.cpp
// enumerates it at its seams and prints plans that tests/test_route_plan_cpu.py compares with tests/route_model.py).
#pragma once
#include <cstdint>
#include <initializer_list>

namespace d2pc {

constexpr int kBlock = 256;  // threads per workgroup (4 waves of 64)
constexpr uint32_t kCbMaxTilesX = 128;  // tiles per band: far below the blocks resident at once (3 per CU)
constexpr int kResidentBlocksPerCu = 4;  // what k_compact_resident's grid may be at most, per CU (<= 128 VGPRs: admitted)

namespace host {

constexpr int kDefaultOnepassForm = 2;  // profiles/r05_ab_onepass_forms_*.txt: never slower than form 1, 5-6 % faster with 30 % holes, 29 % with 90 %

// the big-batch seam (see plan_compact)
constexpr uint32_t kBigBatchFrames = 4, kBigBatchTiles = 20480;
// tiles of one frame the resident blocks serve: a block sums its frame's lower-numbered blocks in one pass of its threads
constexpr uint32_t kResidentMaxTilesPerFrame = 1024;
// the single pass: frames of this many tiles or more run with 3 blocks per CU, shorter ones with 4 (see plan_compact)
constexpr uint32_t kOnepassLongFrameTiles = 2048;
// 8- / 16-bit PARITY launches of this many ROI pixels or more take one pixel per thread (see parity_pxt)
constexpr long long kParityOnePixelFrom = 96000000ll;
// the chunked overlap of the callback body: every chunk carries at least this many pixels (see plan_callback)
constexpr uint64_t kCbChunkMinPixels = uint64_t(16) << 20;
// the ramped start of k_compact_resident_lean (see plan_compact): bytes per second, shader clock, cycles per sleep, the
// fixed point of Geom::stagger; the default scale in %; the fill of the resident capacity from which it is applied
constexpr double kRampBytesPerSec = 6.0e12, kRampClockHz = 2.4e9, kRampSleepCycles = 64.0, kRampFixedPoint = 1024.0;
constexpr int kRampDefaultPct = 50;
constexpr uint32_t kRampFillNum = 7, kRampFillDen = 8;

// PARITY tile shape.  Default (round 3): ONE-SHOT blocks of 512 pixels, two per thread (k_reproject_pack_small) -- against
// the tile-walking kernel with 8 pixels per thread, interleaved on one device: 16 x 4K 427 -> 394 us (border 40), 457 -> 407 us
// (border 0); one 4K frame 24.9 -> 23.0 us; 64 x 752x480 51.2 -> 49.6 us; never slower (profiles/r03_sweep_parity_small.txt).
// One pixel per thread is as good for fp32 launches that fit the caches and 15 % worse for the big fp32 batch.
// 8- and 16-bit input -- what the reference's callback really holds (cpp:60-61) -- swept in round 4
// (profiles/r04_sweep_parity_small_u8.txt): two pixels per thread up to ~8 x 4K (2 x 4K: 38.1 against 45.5 us), ONE pixel per
// thread beyond (16 x 4K: u8 281.6 against 313.0 us, u16 298.2 against 325.7; equal at 8 x 4K).
// pxt_parity 4 / 8 / 16 select the tile-walking kernel (1024-pixel tiles were its best for launches of <= 32 Mpixel).
inline int parity_pxt(int pxt_parity, bool is_f32, int border, int width, int height, int n_frames) {
  if (pxt_parity) return pxt_parity;
  if (is_f32) return 2;
  const long long b = border, rw = (long long)width - 2 * b, rh = (long long)height - 2 * b;
  const long long px = rw > 0 && rh > 0 ? rw * rh * (long long)n_frames : 0;
  return px >= kParityOnePixelFrom ? 1 : 2;
}

// tiles of 256 * pxt ROI pixels in a frame of roi_n
inline uint32_t tiles_of(uint32_t roi_n, int pxt) {
  const uint32_t tile_px = uint32_t(kBlock) * uint32_t(pxt);
  return (roi_n + tile_px - 1) / tile_px;
}

// grid: many more blocks than fit (the dispatcher keeps the CUs fed as blocks
// retire), each walking a few tiles: min(T, max(CUs*blocks_per_cu, T/4))
inline uint32_t walk_grid(uint32_t total_tiles, int cu, int blocks_per_cu) {
  uint32_t want = uint32_t(cu) * uint32_t(blocks_per_cu);
  const uint32_t quarter = (total_tiles + 3) / 4;
  if (want < quarter) want = quarter;
  const uint32_t grid = total_tiles < want ? total_tiles : want;
  return grid ? grid : 1;
}

// blocks resident at once for the resident forms (compact_algo 3)
inline uint32_t resident_cap(int cu) { return uint32_t(cu * kResidentBlocksPerCu); }

// Do n_frames frames of roi_n pixels fit the resident blocks at r pixels per thread: every tile a block of its own, all
// resident at once, a frame of at most 1,024 of them.
// EXPERIMENT "resident_unbounded": more blocks than fit at once.  A block waits for lower-numbered blocks of its frame
// only, so this is safe exactly if every XCD starts its share of the grid in index order (then the lowest unfinished
// block always runs); the time-out turns a violation into kCountTimedOut, not a hang
inline bool resident_fit(uint32_t roi_n, uint32_t n_frames, int r, uint32_t cap, bool unbounded = false) {
  const uint32_t tpf = tiles_of(roi_n, r);
  const uint64_t blocks = uint64_t(tpf) * n_frames;
  const bool fits = blocks <= cap || (unbounded && r >= 32 && blocks <= 0x7fffffffull);
  return fits && (tpf <= kResidentMaxTilesPerFrame || unbounded);
}

// The tuning fields the routing reads (d2pc_ctx; d2pc_set_tuning) and the device's CU count.
struct RouteTuning {
  int cu_count;
  int compact_algo;  // d2pc_config::compact_algo: 0 = choose per launch
  int blocks_per_cu, onepass_blocks_per_cu, onepass_form;
  int resident_pxt, resident_pair, resident_unbounded, resident_stagger_pct;
  int big_batch_algo, chunk_mb, chunk_first_frames;
};

// One COMPACT launch as enqueue receives it.
struct CompactCall {
  uint32_t roi_n, n_frames;
  int pxt;        // the caller's tiles (pxt_compact)
  int elem_size;  // bytes per input sample
  bool is_f32;
  bool captured;  // the stream is being captured
  int force_algo;
};

struct CompactPlan {
  bool split;           // two one-frame launches, back to back; nothing else of the plan counts then
  int algo;             // 1 two-pass, 2 single pass, 3 resident blocks, 4 chunked two-pass (experiment build)
  int pxt;              // pixels per thread of the tiles the launch runs in
  int onepass_form;     // algo 2
  uint32_t grid;
  uint32_t stagger;     // algo 3, register-resident form: Geom::stagger
  bool lean;            // algo 3 in other tiles than the caller's: k_compact_resident_lean
  bool self_clean;      // the launch zeroes the idle half of its state buffer for its successor
  uint32_t chunk_frames, chunk_first;  // algo 4
};

// The pixels per thread at which the launch is resident-routable, 0 if at none: the ordinary tiles, else 32, else 64;
// tuning "resident_pxt" forces one of the shapes where it fits.
inline int resident_shape(const RouteTuning &t, const CompactCall &c) {
  const uint32_t cap = resident_cap(t.cu_count);
  if (t.resident_pxt) return resident_fit(c.roi_n, c.n_frames, t.resident_pxt, cap, t.resident_unbounded != 0) ? t.resident_pxt : 0;
  for (int r : {c.pxt, 32, 64})
    if (resident_fit(c.roi_n, c.n_frames, r, cap)) return r;
  return 0;
}

inline CompactPlan plan_compact(const RouteTuning &t, const CompactCall &c) {
  CompactPlan p{};
  const uint32_t cap = resident_cap(t.cu_count);
  const uint32_t tpf = tiles_of(c.roi_n, c.pxt), total = uint32_t(uint64_t(tpf) * c.n_frames);
  // TWO frames that fit the resident blocks only as one launch of 16,384-pixel blocks (two 4K frames): two launches of
  // 8,192-pixel blocks, back to back on the stream, instead.  Measured on the driver's device in round 4: 65.6 us for the
  // pair in one launch (every block twice as long in its read-then-write chain, no ramped start: 9 us of waiting per block)
  // against 2 x 27.0 us; the back-to-back launches leave no gap since the buffers' events are recorded lazily.
  // Tuning "resident_pair" = 1 keeps the one launch (tools/ab_resident.sh).
  if (c.n_frames == 2 && !c.force_algo && (t.compact_algo == 0 || t.compact_algo == 3) && !t.resident_pxt && !t.resident_pair &&
      !c.captured) {
    // the resident routing's own test below, for ONE frame at up to 32 pixels per thread (tpf <= 1024 included: on a device
    // of more CUs a single frame could otherwise fall to two two-pass launches, slower than the one launch it replaced), and
    // the pair fits neither in the ordinary tiles nor at 32 pixels per thread
    const bool single_is_resident32 = resident_fit(c.roi_n, 1, c.pxt, cap) || resident_fit(c.roi_n, 1, 32, cap);
    if (2u * tpf > cap && 2u * tiles_of(c.roi_n, 32) > cap && single_is_resident32) {
      p.split = true;
      return p;
    }
  }
  // default (0): the single pass (one read of the input) wins once a launch is big enough to amortise
  // its pipeline fill -- measured crossover ~25k tiles (16 x 4K: 449 vs 495 us; 32 x 1080p: 196 vs 207;
  // 256 x 752x480: 278 vs 290; but 8 x 1080p: 68 vs 61) -- and needs a few frames in flight, because a
  // frame's ticket word serialises at ~18 ns per tile (one 4K frame: 72 vs 35 us)
  // (round 4, profiles/r04_ab_midrange.txt: the crossover is where the input stops fitting the Infinity Cache between the two-pass
  // form's two reads, ~160 MB = ~20k tiles of fp32 -- 6 x 4K (22.9k tiles): single pass 166 us, two-pass 184; 4 x 4K (15.3k): 117 / 114;
  // 16 x 1080p (14.4k): 112 / 103.  The threshold was 24,576 before, which sent 6 x 4K the slower way.)
  const bool big_batch = c.n_frames >= kBigBatchFrames && total >= kBigBatchTiles;
  // camera-size launches whose tiles are all resident at once take ONE launch (k_compact_resident) unless the call
  // is being captured (its epoch argument would freeze in the graph); one 1080p frame 16 -> ~8 us
  // ... in the ordinary tiles (k_compact_resident), or -- one or two 4K frames -- in blocks of 32 / 64 pixels per thread
  // that keep their disparities in registers between count and scatter (k_compact_resident_lean)
  const int resident_pxt = resident_shape(t, c);
  const bool resident_ok = resident_pxt != 0 && !c.captured;
  const int dflt = big_batch ? t.big_batch_algo : resident_ok ? 3 : 1;
  p.algo = c.force_algo ? c.force_algo : t.compact_algo ? t.compact_algo : dflt;
  if (p.algo == 3 && !resident_ok) p.algo = big_batch ? t.big_batch_algo : 1;  // (asked for, not possible here)
  p.pxt = c.pxt;
  p.grid = walk_grid(total, t.cu_count, t.blocks_per_cu);  // (the two-pass forms, 1 and 4)
  if (p.algo == 3) {
    p.pxt = resident_pxt;
    p.grid = uint32_t(uint64_t(tiles_of(c.roi_n, resident_pxt)) * c.n_frames);
    p.lean = resident_pxt != c.pxt;
    if (p.lean) {
      // the ramped start of k_compact_resident_lean: a block's input bytes at ~6 TB/s and ~2.4 GHz, in 64-cycle sleeps x 1024
      // (R = 32, fp32: 32 KiB per block = 13 cycles = 0.2 sleeps per block index); tuning "resident_stagger_pct" scales it
      // Measured (profiles/r04_ab_stagger.txt): half that ramp is worth 1.4-1.8 us on ONE 4K frame (31.2 -> 29.8 us with 30 % holes
      // + indices, 32.2 -> 30.4 all valid) and nothing or less on two frames and on smaller ones, whose blocks do not fill the
      // device: it is applied to single frames of >= 7/8 of the resident capacity only.
      const double block_bytes = double(kBlock) * resident_pxt * double(c.elem_size);
      const bool ramp = t.resident_stagger_pct >= 0 ? true : (c.n_frames == 1 && c.is_f32 && p.grid * kRampFillDen >= cap * kRampFillNum);
      const int pct = t.resident_stagger_pct >= 0 ? t.resident_stagger_pct : kRampDefaultPct;
      p.stagger = ramp ? uint32_t(block_bytes / kRampBytesPerSec * kRampClockHz / kRampSleepCycles * kRampFixedPoint * pct / 100.0) : 0u;
    }
  }
  if (p.algo == 4) {
    // chunked two-pass (k_compact_chunk): the geometry in its own 512-pixel tiles; chunks of whole frames whose input
    // stays in the Infinity Cache between the launch that counts it and the launch that scatters it
    p.pxt = 2;
    const uint64_t frame_bytes = uint64_t(c.roi_n) * uint64_t(c.elem_size);
    uint64_t per = (uint64_t(t.chunk_mb) << 20) / (frame_bytes ? frame_bytes : 1);
    if (per < 1) per = 1;
    if (per > c.n_frames) per = c.n_frames;
    p.chunk_frames = uint32_t(per);
    // the first chunk is counted with nothing to run beside it: an eighth of a chunk (a 4K stream: one frame)
    p.chunk_first = t.chunk_first_frames > 0 ? uint32_t(t.chunk_first_frames) : uint32_t((per + 7) / 8);
    if (p.chunk_first > p.chunk_frames) p.chunk_first = p.chunk_frames;
  }
  if (p.algo == 2) {
    // the single-pass kernel is software-pipelined over a block's tiles: it
    // wants few, long-lived blocks (about what is resident), not many short ones
    // interleaved sweeps on two devices (profiles/r02_ab_onepass_v2_vs_r1.txt): 4K frames run 1-3 % faster with 3
    // blocks per CU (fewer failed polls), 1080p-class frames 1-4 % faster with 4
    // which single-pass kernel (tuning "onepass_form"; same bytes out): 2 = the count phase packs the survivors, the scatter
    // phase runs dense (round 5: the product's); experiment build: 1 = raw tiles in LDS, every pixel decided in both phases
    // (rounds 2-4), 3 = form 2 with 8 worker waves on tiles of 4,096 pixels, 4 = form 2 with the control wave as the loader
    // 5 = form 2 with 4 runs per worker wave (4,096-pixel tiles), 6 = form 2 with deferred landing (a tile's loads fly for a
    // whole iteration), 7 = 5 + 6: profiles/r05_ab_forms567.txt
    p.onepass_form = t.onepass_form ? t.onepass_form : kDefaultOnepassForm;
    const bool big_tiles = p.onepass_form == 3 || p.onepass_form == 5 || p.onepass_form == 7;
    p.pxt = big_tiles ? 16 : p.onepass_form >= 2 ? 8 : c.pxt;
    const uint32_t form_tpf = tiles_of(c.roi_n, p.pxt), form_total = uint32_t(uint64_t(form_tpf) * c.n_frames);
    const int dflt_per_cu = big_tiles ? 2 : (form_tpf >= kOnepassLongFrameTiles ? 3 : 4);
    const int per_cu = t.onepass_blocks_per_cu ? t.onepass_blocks_per_cu : dflt_per_cu;
    const uint32_t persistent = uint32_t(t.cu_count) * uint32_t(per_cu);
    p.grid = form_total < persistent ? form_total : persistent;
    if (p.grid < c.n_frames) {  // more frames than blocks: every block serves one frame only
      p.algo = 1;
      p.pxt = c.pxt;
      p.grid = walk_grid(total, t.cu_count, t.blocks_per_cu);
    }
  }
  // the dense single pass cleans up for its successor: two states per buffer (see StateBuf::pp_*)
  p.self_clean = p.algo == 2 && p.onepass_form >= 2 && p.onepass_form != 4;  // (every dense form)
  return p;
}

// ---- the callback body (d2pc_process_mono_device) ---------------------------------------------------------------------
inline uint32_t cb_tiles_x(uint32_t roi_w) { return (roi_w + 255u) / 256u; }  // tiles of 256 x 32 ROI pixels
inline uint32_t cb_tiles_y(uint32_t roi_h) { return (roi_h + 31u) / 32u; }

struct CallbackTuning {
  int cb_chunks, cb_fused, cb_fused_compact;
};
struct CallbackCall {
  int width, height, n_frames;
  bool median, bridge16;  // a median filter / the mono16 rescale runs in front of the reprojection
  bool captured;          // the stream is being captured
  bool compact;
  bool bs_median;         // the bit-sliced median would serve the filter launch of the whole batch (median_uses_bs)
  uint32_t roi_w;
};
struct CallbackPlan {
  bool overlap;     // chunks of the batch: the filter of one on one stream beside the reprojection of another
  int chunk;        // frames per chunk (n_frames: the batch in order on the caller's stream)
  bool one_kernel;  // filter + points tile by tile in one kernel, which needs no filtered frames
};

inline CallbackPlan plan_callback(const CallbackTuning &t, const CallbackCall &c) {
  CallbackPlan p{};
  // Few, large chunks: a cross-stream dependency costs ~20 us on this runtime (measured: 16 one-frame chunks of
  // 4K frames are 19 % SLOWER than running in order, 2 chunks 8 % faster), so the batch is only cut when every
  // chunk carries well over that in kernel time
  const uint64_t batch_px = uint64_t(c.width) * uint64_t(c.height) * uint64_t(c.n_frames);
  const int n_chunks = t.cb_chunks > c.n_frames ? c.n_frames : t.cb_chunks;
  p.overlap = n_chunks > 1 && !c.captured && (c.median || c.bridge16) && batch_px / uint64_t(n_chunks) >= kCbChunkMinPixels;
  p.chunk = p.overlap ? (c.n_frames + n_chunks - 1) / n_chunks : c.n_frames;
  // Can the tile-fused kernel (median + points per tile) serve this call?  COMPACT: a band of tiles must fit the
  // blocks resident at once (k_callback_bs_compact's hand-off), i.e. ROIs up to 128 x 256 pixels wide.
  const bool fused_ok = !c.compact || (t.cb_fused_compact >= 1 && cb_tiles_x(c.roi_w) <= kCbMaxTilesX);
  p.one_kernel = c.median && t.cb_fused == 1 && !p.overlap && c.bs_median && fused_ok;
  return p;
}

// Residency of the fused COMPACT callback kernels.  Both forms of the kernel hand counts over between the tiles of a BAND,
// and a frame's blocks are dispatched round-robin over the launch's frames (frame = blockIdx % n_frames): a frame needs
// tiles_x of its own blocks resident at once, or no frame ever finishes band 0 (advisor, round 3: from ~385 frames of 752x480
// or ~55 frames of 4K every wave spun out its 4-s budget).  A call with more frames than that is cut into
// sub-batches of nfc frames with resident / nfc > tiles_x, launched back to back on the same stream (they share
// the stream's state buffer: a sub-batch's zeroing kernel runs behind the previous sub-batch's last store).
struct CallbackCompactPlan {
  uint32_t tiles_x, tpf;
  uint32_t resident;     // blocks resident at once
  uint32_t nfc;          // frames per sub-batch
  uint32_t sub_batches;  // launches that serve the call's frames, nfc at a time
  bool pipe;             // cb_fused_compact 2: the pipelined form where a sub-batch admits it

  struct Sub {
    uint32_t per_frame, grid;
    bool pipelined;  // else the one-tile-per-block form, whose grid is the launch's own (tiles x frames)
  };
  // a sub-batch of ns <= nfc frames
  Sub sub(uint32_t ns) const {
    Sub s{tpf, tpf * ns, false};
    if (pipe) {
      // persistent blocks, a multiple of the frame count; every frame needs more blocks than a band has tiles
      // (or as many as it has tiles): otherwise the one-tile-per-block form serves the launch
      uint32_t per_frame = resident / ns;
      if (per_frame > tpf) per_frame = tpf;
      if (per_frame > tiles_x || per_frame == tpf) s = Sub{per_frame, per_frame * ns, true};
    }
    // (the one-tile-per-block form: ns * tiles_x <= resident - ns by the choice of nfc, so every frame has a whole
    // band of blocks resident from the first dispatch round on)
    return s;
  }
};

inline CallbackCompactPlan plan_callback_compact(int cu, int per_cu, int cb_fused_compact, uint32_t tiles_x, uint32_t tiles_y,
                                                 uint32_t n_frames) {
  CallbackCompactPlan p{};
  p.tiles_x = tiles_x;
  p.tpf = tiles_x * tiles_y;
  p.resident = uint32_t(cu * (per_cu < 3 ? per_cu : 3));  // (LDS and registers admit 3 per CU)
  p.nfc = p.resident / (p.tiles_x + 1u);  // (tiles_x <= kCbMaxTilesX = 128 < resident: nfc >= 1 on any device of >= 43 CUs)
  if (p.nfc == 0) p.nfc = 1;
  p.sub_batches = (n_frames + p.nfc - 1) / p.nfc;
  p.pipe = cb_fused_compact == 2;
  return p;
}

}  // namespace host
}  // namespace d2pc
