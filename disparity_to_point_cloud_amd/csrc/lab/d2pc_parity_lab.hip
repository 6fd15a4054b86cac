// lab/d2pc_parity_lab.hip -- EXPERIMENT BUILD ONLY (-DD2PC_EXPERIMENTS=1): PARITY by tiles that fewer, longer-lived blocks
// walk (rounds 1-2; tuning key pxt_parity 4 / 8 / 16).  The product's one-shot blocks: ../d2pc_parity.hip.
#include "../d2pc_pixel.hpp"

namespace d2pc {

// --------------------------------------------------------------------------
// K1: PARITY mode -- every ROI pixel, reference order, nothing filtered.
// --------------------------------------------------------------------------
template <int DT, int QK, int PXT, bool VEC>
__global__ __launch_bounds__(kBlock) void k_reproject_pack(const uint8_t *__restrict__ disp,
                                                           float4 *__restrict__ out,
                                                           uint32_t *__restrict__ out_index,
                                                           uint32_t *__restrict__ counts, const Geom g,
                                                           const QArg<QK> Q) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  D2PC_DECLARE_STRIPS(VEC, wave);
  for (uint32_t t = blockIdx.x; t < g.total_tiles; t += gridDim.x) {
    const uint32_t f = fdiv(t, g.div_tpf);
    const uint32_t lt = t - f * g.tiles_per_frame;
    const uint8_t *fin = disp + uint64_t(f) * g.in_frame_stride;
    float4 *fout = out + uint64_t(f) * g.out_frame_stride;
    uint32_t *fidx = out_index ? out_index + uint64_t(f) * g.out_frame_stride : nullptr;
    const uint32_t base = lt * uint32_t(kBlock * PXT);
    TileRegs<DT, QK, PXT> r;
    tile_compute<DT, QK, PXT, VEC>(r, fin, g, Q, base, wave, lane, wave_strip);
#pragma unroll
    for (int k = 0; k < PXT; ++k) {
      const uint32_t i = slot_pixel(base, wave, lane, k);
      if (i < g.roi_n) {
        store_point<D2PC_STORE_NT != 0>(fout, i, r.X[k], r.Y[k], r.Z[k]);
        if (fidx) store_index(fidx, i, r.pix[k]);
      }
    }
    if (counts && lt == 0 && tid == 0) counts[f] = g.roi_n;
  }
}

template <int PXT>
static hipError_t launch_walking(const LaunchArgs &a) {
  return for_q_kind(a.q_kind, [&](auto qk) {
    return for_dtype_vec(a, [&](auto dt, auto vec) {
      constexpr int QK = decltype(qk)::value, DT = decltype(dt)::value;
      constexpr bool VEC = decltype(vec)::value;
      hipLaunchKernelGGL((k_reproject_pack<DT, QK, PXT, VEC>), dim3(a.grid), dim3(kBlock), 0, a.stream,
                         static_cast<const uint8_t *>(a.disp), static_cast<float4 *>(a.out_points), a.out_index, a.counts, a.geom,
                         make_qarg<QK>(a));
      return hipGetLastError();
    });
  });
}

// launch_parity (d2pc_parity.hip) without parity_small
hipError_t launch_parity_lab(const LaunchArgs &a) {
  switch (a.pxt) {
    case 4: return launch_walking<4>(a);
    case 8: return launch_walking<8>(a);
    case 16: return launch_walking<16>(a);
  }
  return hipErrorInvalidValue;
}

}  // namespace d2pc
