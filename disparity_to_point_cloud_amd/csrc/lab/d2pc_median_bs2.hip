// lab/d2pc_median_bs2.hip -- EXPERIMENT BUILD ONLY (-DD2PC_EXPERIMENTS=1): the bit-sliced median with the select split over
// a lane pair, as a kernel of its own (median_algo 3; tile body and design notes: d2pc_median_bs2_tile.hpp).  The
// product's kernel: ../d2pc_median_bs.hip.
#include "d2pc_median_bs2_tile.hpp"
#include "../d2pc_pixel.hpp"

namespace d2pc {

// the lane-pair form of the select (d2pc_median_bs2_tile.hpp, select2): 512 threads per tile, four waves per SIMD
template <int KS>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_median_bs2_u8(
    const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const MedianArgs a) {
  using S = MedianBsShape<KS>;
  __shared__ __attribute__((aligned(16))) uint32_t s_w[S::W_WORDS];
  __shared__ __attribute__((aligned(16))) uint32_t s_raw[S::RAW_WORDS];
  const uint32_t tid = threadIdx.x;
  uint32_t b = blockIdx.x;
  const uint32_t f = b / (a.tiles_x * a.tiles_y);
  b -= f * a.tiles_x * a.tiles_y;
  const uint32_t ty = b / a.tiles_x, tx = b - ty * a.tiles_x;
  const int x0 = int(a.out_x0) + int(tx) * S::TW, y0 = int(a.out_y0) + int(ty) * S::TH;
  median_bs2_tile<KS>(src + uint64_t(f) * a.src_frame_stride, a, x0, y0, s_w, s_raw, tid);
  uint8_t *fdst = dst + uint64_t(f) * a.dst_frame_stride;
  const uint8_t *ob = reinterpret_cast<const uint8_t *>(s_w);
  const uint32_t x_end = a.out_x0 + a.out_w, y_end = a.out_y0 + a.out_h;
  for (uint32_t c = tid; c < uint32_t(S::TW * S::TH / 16); c += 512u) {
    const uint32_t r = c / uint32_t(S::TW / 16), xo = 16u * (c - r * uint32_t(S::TW / 16));
    const uint32_t oy = uint32_t(y0) + r, ox = uint32_t(x0) + xo;
    if (oy >= y_end || ox >= x_end) continue;
    uint8_t *o = fdst + uint64_t(oy) * a.dst_row_stride + ox;
    const uint8_t *i = ob + r * uint32_t(S::OUT_STRIDE) + xo;
    if (ox + 16u <= x_end) {
      __builtin_memcpy(o, i, 16);
    } else {
      for (uint32_t k = 0; ox + k < x_end; ++k) o[k] = i[k];
    }
  }
}

// `a` arrives from launch_bs (d2pc_median_bs.hip) with its tiles counted: `blocks` of them over all frames
hipError_t launch_median_bs2(const uint8_t *src, uint8_t *dst, const MedianArgs &a, int ksize, uint32_t blocks, hipStream_t stream) {
  return for_ksize(ksize, [&](auto ks) {
    hipLaunchKernelGGL(k_median_bs2_u8<decltype(ks)::value>, dim3(blocks), dim3(512), 0, stream, src, dst, a);
    return hipGetLastError();
  });
}

}  // namespace d2pc
