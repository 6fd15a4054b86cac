// d2pc_onepass_run.hpp -- what the single-pass COMPACT kernels share (protocol and pipeline: d2pc_onepass.hip): validity
// and points of one run of 256 pixels, the control wave's scan of a tile's run counts, and the three epilogues of the
// protocol (publish a tile, report a frame's count, flush the block's counters).  Used by k_compact_onepass_dense
// (d2pc_onepass.hip) and, in the experiment build, by forms 1 and 4 (lab/d2pc_onepass_lab.hip).
#pragma once

#include "d2pc_compact_common.hpp"

namespace d2pc {

// ---- single-pass building blocks: validity and points of one wave's share of a tile -------------------

// Exact validity of pixel i by the real arithmetic (general Q, and tiles with a sliver).
template <int QK>
__device__ __forceinline__ bool pixel_valid_exact(const QArg<QK> &Q, const Geom &g, uint32_t i, float d) {
  uint32_t uu, vv;
  pixel_coords(g, i, uu, vv);
  float X, Y, Z;
  reproject(Q, uu, vv, d, X, Y, Z);
  return point_is_valid(X, Y, Z, d, g.min_disparity);
}

// A wave-uniform pointer moved into vector registers: the single-pass kernel runs out of scalar registers,
// and a spilled scalar base costs a v_readlane pair before every store.  With the base in VGPRs the store
// address is one v_lshl_add_u64.
__device__ __forceinline__ uint64_t vgpr_pointer(const void *p) {
  const uint64_t x = reinterpret_cast<uint64_t>(p);
  uint32_t lo, hi;
  asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=&v"(lo), "=v"(hi) : "s"(uint32_t(x)), "s"(uint32_t(x >> 32)));
  return (uint64_t(hi) << 32) | lo;
}

// inclusive scan of up to 16 cells held one per lane (lanes 0 .. CELLS-1 of a DPP row): three or four row shifts, no LDS
template <int CELLS>
__device__ __forceinline__ uint32_t scan_row(uint32_t c, uint32_t &total) {
  static_assert(CELLS <= 16, "one DPP row");
  uint32_t incl = c;
  incl += uint32_t(__builtin_amdgcn_update_dpp(0, int(incl), 0x111, 0xf, 0xf, false));  // row_shr:1
  incl += uint32_t(__builtin_amdgcn_update_dpp(0, int(incl), 0x112, 0xf, 0xf, false));  // row_shr:2
  incl += uint32_t(__builtin_amdgcn_update_dpp(0, int(incl), 0x114, 0xf, 0xf, false));  // row_shr:4
  if (CELLS > 8) incl += uint32_t(__builtin_amdgcn_update_dpp(0, int(incl), 0x118, 0xf, 0xf, false));  // row_shr:8
  total = uint32_t(__builtin_amdgcn_readlane(int(incl), CELLS - 1));
  return incl;
}

// Count phase of one run: decides its 256 pixels (the exact predicate of tile_count; the real arithmetic for a general Q
// or a run that holds a sliver), packs the survivors' disparities to the front of the run's slice IN PLACE (all four
// slots are read before the first is written, and a survivor's rank never exceeds its pixel's offset; LDS is in-order
// per wave) with their offsets inside the run beside them, and returns the survivors' number (wave-uniform).
template <int QK>
__device__ __forceinline__ uint32_t run_count_pack(const QArg<QK> &Q, const Geom &g, float *run, uint8_t *off, uint32_t run_base,
                                                   uint32_t lane) {
  float d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) d[k] = run[uint32_t(k) * 64u + lane];
  const uint32_t left = run_base < g.roi_n ? g.roi_n - run_base : 0u;  // pixels of the frame from this run on (ragged: a frame's last tile)
  bool ok[4];
  bool exact = !is_stereo(QK);
  if constexpr (is_stereo(QK)) {
    uint64_t sliver = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double nw = stereo_nw(Q, d[k]);
      const bool fin = finite_nonzero(nw), big = fabs(nw) >= Q.s.w_safe;
      ok[k] = (int(fin) & int(big) & int(!(d[k] <= g.min_disparity)) & int(uint32_t(k) * 64u + lane < left)) != 0;
      sliver |= __ballot(int(fin) & int(!big));
    }
    exact = sliver != 0;
  }
  if (exact) {  // (wave-uniform)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      ok[k] = pixel_valid_exact<QK>(Q, g, run_base + uint32_t(k) * 64u + lane, d[k]) && uint32_t(k) * 64u + lane < left;
  }
  uint32_t c = 0;  // (scalar: survivors of the slots before k)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint64_t m = __ballot(ok[k]);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), c));
    if (ok[k]) {
      run[rank] = d[k];
      off[rank] = uint8_t(uint32_t(k) * 64u + lane);
    }
    c += uint32_t(__popcll(m));
  }
  return c;
}

// Scatter phase of one run: its c survivors, dense, to out[pos0 ...) in order.
template <int QK, bool IDX>
__device__ __forceinline__ void run_scatter_dense(const QArg<QK> &Q, const Geom &g, const float *run, const uint8_t *off, uint32_t c,
                                                  uint32_t pos0, uint32_t run_base, uint32_t lane, uint64_t fout, uint64_t fidx) {
  // the run's first pixel (wave-uniform: scalar arithmetic); a run of 256 pixels wraps at most once when the ROI is at
  // least 256 pixels wide, and takes the division per pixel otherwise
  const uint32_t v0 = fdiv(run_base, g.div_roi_w), u0 = run_base - v0 * g.roi_w;
  const bool wide = g.roi_w >= 256u;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (uint32_t(s) * 64u >= c) break;  // (wave-uniform)
    // (starting every store instruction on a 64-byte line of the output -- the run's first pos0 & 3 lanes idle, 16 whole
    // lines per instruction instead of 17 partial ones -- changes nothing: L2 merges the shared end lines of plain stores;
    // profiles/r05_ab_dense_variants.txt)
    const uint32_t j = uint32_t(s) * 64u + lane;
    const float d = run[j];       // (lanes past c read what the pack left there: computed, never stored)
    const uint32_t o = off[j];
    uint32_t u, v;
    if (wide) {
      u = u0 + o;
      v = v0;
      if (u >= g.roi_w) u -= g.roi_w, v += 1u;
    } else {
      const uint32_t i = run_base + o;
      v = fdiv(i, g.div_roi_w);
      u = i - v * g.roi_w;
    }
    const uint32_t uu = u + g.border, vv = v + g.border;
    float X, Y, Z;
    if constexpr (is_stereo(QK)) {  // (a survivor's d is finite: reproject()'s poisoning of a non-finite d has nothing to do)
      const double iw = 1.0 / stereo_nw(Q, d);
      X = float(stereo_nx(Q, uu) * iw);
      Y = float(stereo_ny(Q, vv) * iw);
      Z = big_z_rule(d, float(Q.s.f * iw));
    } else {
      reproject(Q, uu, vv, d, X, Y, Z);
    }
    const uint32_t pos = pos0 + j;
    // pos < roi_n always holds for a correct prefix; the guard keeps a stale or timed-out prefix from ever becoming an
    // out-of-bounds store
    if (j < c && pos < g.roi_n) {
      using gv4f = __attribute__((address_space(1))) v4f;
      using gu32 = __attribute__((address_space(1))) uint32_t;
      const v4f p = {X, Y, Z, 1.0f};
      if (D2PC_ONEPASS_STORE_NT) __builtin_nontemporal_store(p, (gv4f *)(fout + (uint64_t(pos) << 4)));
      else *(gv4f *)(fout + (uint64_t(pos) << 4)) = p;
      if constexpr (IDX) {
        if (D2PC_ONEPASS_INDEX_NT) __builtin_nontemporal_store(vv * g.width + uu, (gu32 *)(fidx + (uint64_t(pos) << 2)));
        else *(gu32 *)(fidx + (uint64_t(pos) << 2)) = vv * g.width + uu;
      }
    }
  }
}

// ---- the protocol's epilogues (one copy for every form) -------------------------------------------------------------

// Publishes tile `tile` of the frame with its `total` survivors: tagged granule (the data is the flag) + group
// accumulator.  (control wave, lane 0)
__device__ __forceinline__ void publish_tile(const FrameState &fs, uint32_t tile, uint32_t total) {
  using gu64 = __attribute__((address_space(1))) uint64_t;
  __hip_atomic_store((gu64 *)(fs.granules + 2u * tile), kGranuleTag | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add((gu64 *)fs.group_word(tile / kGroupTiles), (uint64_t(1) << 32) | total, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// Frame f's count at a block's end: a block that saw the launch break marks the frame it was serving kCountTimedOut (it
// may have scattered with a prefix it never obtained), whether or not the frame's last tile has reported its count
// already.  (one thread.  The last tile's own report -- the same rule around the count -- stays written out in each
// kernel: as a function, its count argument is evaluated ahead of the flag's load instead of inside the choice, and
// every single-pass kernel's code came out different, most by one instruction.)
__device__ __forceinline__ void report_timeout(uint32_t *counts, uint32_t f, StateHeader *hdr) {
  if (__hip_atomic_load(&hdr->timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    __hip_atomic_store(counts + f, kCountTimedOut, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The block's share of the context's counters (s_stat: PollStats' three words): no-return atomics, once per block, on the
// block's slot (one word for all blocks serialised the launch's end: d2pc_device.hpp).  (control wave, lane 0)
__device__ __forceinline__ void flush_block_stats(StateHeader *hdr, const uint32_t *s_stat) {
  CompactStats::Slot *sl = hdr->stats->slot + (blockIdx.x % uint32_t(kStatSlots));
  atomicAdd(&sl->tiles, (unsigned long long)s_stat[0]);
  if (s_stat[1]) {
    atomicAdd(&sl->failed_polls, (unsigned long long)s_stat[1]);
    atomicAdd(&sl->wait_ticks, (unsigned long long)s_stat[2]);
  }
}

}  // namespace d2pc
