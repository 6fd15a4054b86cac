// d2pc_sectors_slope_fit.hpp -- what the slope's kernels (d2pc_sectors_slope.hip) and the relief's (d2pc_sectors_relief.hip)
// share on the device, each written once: the SLOPE block's fit of one cell from its count and nine sums, and the site stage
// with the number of fitted cells over the summary's word 3.
// Device code: a .hip file includes it.  The fit is one fixed sequence of double operations, each rounded once: contraction
// is off inside it whatever the including file sets.
#pragma once
#include <hip/hip_runtime.h>

#include "d2pc_sectors_ground_sites.hpp"
#include "d2pc_sectors_slope_plan.hpp"

namespace d2pc {
namespace sectors {

struct SlopeFit {   // what the fit reads of the two configurations
  uint32_t min_fit, max_spread_q2;   // min_fit = max(min_count, 3)
  double scale, max_tilt2;
};

inline SlopeFit slope_fit_of(const SlopePlan &p) {
  SlopeFit f;
  f.min_fit = p.ground.min_count > 3u ? p.ground.min_count : 3u, f.max_spread_q2 = p.ground.max_spread_q2;
  f.scale = p.scale, f.max_tilt2 = p.max_tilt2;
  return f;
}

// what the fit makes of a cell
struct SlopeCell {
  uint32_t slope_a, slope_b, level_q, resid_q2;   // the floats as bits
  uint8_t flat, fitted;
};

// The SLOPE block's fit of one cell from its count and nine sums s[] (sum, sum2, su, sw, suu, suw, sww, suk, swk).
__device__ __forceinline__ SlopeCell slope_cell_fit(const SlopeFit &a, uint32_t cnt, const unsigned long long (&s)[kSlopeWords]) {
#pragma clang fp contract(off)
  SlopeCell o;
  uint32_t mean, spread;
  ground_cell_formula(cnt, s[0], s[1], &mean, &spread);   // (d2pc_sectors_ground_sites.hpp: m and floor(S / count), the empty cell's words)
  o.slope_a = o.slope_b = D2PC_SECTORS_SLOPE_NOT_FITTED, o.level_q = mean, o.resid_q2 = spread, o.flat = 0, o.fitted = 0;
  if (cnt == 0u) return o;
  // the integer pre-steps, wrapping
  const unsigned long long um = static_cast<unsigned long long>(static_cast<long long>(int(mean))), uc = cnt;
  const unsigned long long uS = s[1] - 2ull * um * s[0] + uc * um * um;
  const double N = double(cnt), S = double(uS);
  const double r = double(static_cast<long long>(s[0] - uc * um));
  const double su = double(static_cast<long long>(s[2])), sw = double(static_cast<long long>(s[3]));
  const double suu = double(static_cast<long long>(s[4])), suw = double(static_cast<long long>(s[5])), sww = double(static_cast<long long>(s[6]));
  const double suk = double(static_cast<long long>(s[7] - um * s[2])), swk = double(static_cast<long long>(s[8] - um * s[3]));
  const double A = N * suu - su * su, B = N * suw - su * sw, C = N * sww - sw * sw;
  const double E = N * suk - su * r, F = N * swk - sw * r, G = N * S - r * r;
  const double AC = A * C;
  const double D = AC - B * B;
  if (!(cnt >= a.min_fit && AC > 0.0 && D * 1048576.0 > AC)) return o;
  const double gu = (E * C - F * B) / D, gw = (F * A - E * B) / D;
  const double Q = (G - gu * E) - gw * F, c0 = ((r - gu * su) - gw * sw) / N;
  const double sa = gu * a.scale, sb = gw * a.scale;
  double rc = rint(c0);
  rc = rc < -2147483648.0 ? -2147483648.0 : (rc > 2147483647.0 ? 2147483647.0 : rc);
  const double mq = floor((Q > 0.0 ? Q : 0.0) / (N * N));
  o.fitted = 1;
  o.slope_a = __float_as_uint(float(sa)), o.slope_b = __float_as_uint(float(sb));
  o.level_q = mean + uint32_t(int(rc));
  o.resid_q2 = mq >= 4294967294.0 ? 0xFFFFFFFEu : uint32_t(mq);
  o.flat = o.resid_q2 <= a.max_spread_q2 && sa * sa + sb * sb <= a.max_tilt2 ? 1 : 0;
  return o;
}

// ground_site_stage for the slope: the stage as it is, then the number of fitted cells over the summary's word 3 (the stage
// stores 0 there from lane 0, which stores again here: one lane, program order).  fit_slot is the caller's, one word a wave,
// filled before the call: the stage's first barrier publishes it.
__device__ __forceinline__ void ground_site_stage(const GroundSiteStage &st, GroundSiteLds &lds, const uint32_t (&spread)[kGroundPerLane],
                                                  uint32_t points, uint32_t n_flat, const uint32_t (&fit_slot)[kGroundSiteWaves]) {
  ground_site_stage(st, lds, spread, points, n_flat);
  if (st.summary && threadIdx.x == 0) {
    uint32_t n_fit = 0;
    for (int w = 0; w < kGroundSiteWaves; ++w) n_fit += fit_slot[w];
    st.summary[3] = n_fit;
  }
}

// The slope's site launch from the 14 bytes per cell that the fitting launch left in hand_on (count, level_q, resid_q2: 4
// bytes x n_cells each, then flat and fitted: n_cells each).  All kGroundSiteThreads lanes call it, under uniform control flow.
__device__ __forceinline__ void slope_sites_from_hand_on(const uint32_t *hand_on, GroundSiteStage &st, GroundSiteLds &lds,
                                                         uint32_t (&fit_slot)[kGroundSiteWaves]) {
  const int tid = int(threadIdx.x);
  const int n_cells = st.grid.n_cells;
  const uint8_t *flat_g = reinterpret_cast<const uint8_t *>(hand_on + 3 * size_t(n_cells));
  uint32_t points = 0, n_flat = 0, n_fit = 0;
  uint32_t resid[kGroundPerLane] = {};
#pragma unroll
  for (int k = 0; k < kGroundPerLane; ++k) {
    const int c = tid + k * kGroundSiteThreads;
    if (c >= n_cells) continue;
    const uint8_t f = flat_g[c];
    points += hand_on[c], n_flat += f, n_fit += flat_g[n_cells + c];
    lds.mean_q[c] = int(hand_on[n_cells + c]), lds.flat[c] = f;
    resid[k] = hand_on[2 * n_cells + c];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) n_fit += uint32_t(__shfl_xor(int(n_fit), m, 64));
  if ((tid & 63) == 0) fit_slot[tid >> 6] = n_fit;
  ground_site_stage(st, lds, resid, points, n_flat, fit_slot);
}

// what the fitting lane hands to the sites
__device__ __forceinline__ void slope_hand_on(uint32_t *hand_on, int n_cells, int cell, uint32_t cnt, const SlopeCell &o) {
  hand_on[cell] = cnt, hand_on[n_cells + cell] = o.level_q, hand_on[2 * n_cells + cell] = o.resid_q2;
  uint8_t *bytes = reinterpret_cast<uint8_t *>(hand_on + 3 * size_t(n_cells));
  bytes[cell] = o.flat, bytes[n_cells + cell] = o.fitted;
}

}  // namespace sectors
}  // namespace d2pc
