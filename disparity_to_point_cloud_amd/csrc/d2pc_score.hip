// d2pc_score.hip -- the matching-score pre-filter of MatchingScoreCb1/2 on gfx950
// (reference src/depth_map_fusion.cpp:64-99):
//   A = GaussianBlur(square view, 13x13, 3)     reads the FRAME's pixels round the square (reflect101 about the frame)
//   M = threshold(Sobel(A, 0,2 | 2,0, ksize 7, scale 0.03), 30) = 255 * (I >= 1017), I the integer Sobel sum
//   B = GaussianBlur(M, 21x21, 10)              reflect101 about the square
//   out = min(255, S + 2 B)                     (grad = B)
// in integers, with the rounding rules of DESIGN.md section 8a (tap tables are launch data; CV4 rounds B half up,
// CV3 half to even; A always rounds half to even).
//
// One tile-fused kernel, no scratch: a workgroup owns a T x T tile of the square and recomputes the halo the chain
// needs in LDS -- 10 pixels of M round the tile, 13 of A, 19 of the frame.  The reflections about the square's
// edges are folded into INDEX MAPS instead of extra passes: every filter of the chain after A is symmetric, so the
// mirror-periodic extension of a filtered image is the filtered mirror-periodic extension, and the tile's M halo
// is computed on "virtual" coordinates v (M_ext(v) = M(refl_n(v))) from A(refl_n(v + j)).  The A rows a tile needs
// are then a contiguous range of square rows, whatever edge the tile touches.
//
// Six separable passes through two LDS buffers (bytes: F, A, M; 16-bit: row sums H, P, Q).  Each thread computes a
// run of kRun outputs along the filter axis from kRun + 2R loads held in registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "d2pc_launch.hpp"

namespace d2pc {

namespace {

constexpr int kSB = 256;  // threads per workgroup
constexpr int kRun = 8;   // outputs per thread and work item of a pass

// cv::borderInterpolate(BORDER_REFLECT_101): the mirror-periodic extension (len >= 2 here: n >= 11, frames >= n)
__device__ __forceinline__ int refl(int p, int len) {
  while (unsigned(p) >= unsigned(len)) p = p < 0 ? -p : 2 * (len - 1) - p;
  return p;
}

// Square rows (or columns) [lo, hi] that refl_n takes over the virtual range [a, b]: a superset, contiguous, of at
// most b - a + 1 entries (a >= 0 unless the tile starts at 0; b - a < n + 26).
__device__ __forceinline__ void refl_span(int a, int b, int n, int &lo, int &hi) {
  if (a >= 0 && b <= n - 1) {
    lo = a, hi = b;
  } else if (a < 0 && b <= n - 1) {
    lo = 0, hi = min(max(b, -a), n - 1);
  } else if (a >= 0) {
    lo = max(min(a, 2 * (n - 1) - b), 0), hi = n - 1;
  } else {
    lo = 0, hi = n - 1;
  }
}

// One separable pass: `lines` independent lines of `outs` outputs, output o reading inputs o .. o + 2R of its line.
// ld(line, i) / st(line, o, sum) hide the layout; consecutive work items take consecutive lines.
template <int R, class Tap, class Ld, class St>
__device__ __forceinline__ void pass(int lines, int outs, Tap tap, Ld ld, St st) {
  const int runs = (outs + kRun - 1) / kRun;
  const int items = lines * runs;
  const int last = outs - 1 + 2 * R;  // the last input index
  for (int it = int(threadIdx.x); it < items; it += kSB) {
    const int run = it / lines, line = it - run * lines;
    const int o0 = run * kRun;
    int v[kRun + 2 * R];
#pragma unroll
    for (int i = 0; i < kRun + 2 * R; ++i) v[i] = ld(line, min(o0 + i, last));
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
      int s = 0;
#pragma unroll
      for (int j = 0; j <= 2 * R; ++j) s += tap(j) * v[k + j];
      if (o0 + k < outs) st(line, o0 + k, s);
    }
  }
}

// rint_even(s / 65536) for s >= 0 (SymmColumnVec_32s8u: float, then cvRound)
__device__ __forceinline__ int round_even16(int s) {
  const int q = s >> 16, r = s & 0xffff;
  return q + int(r > 0x8000 || (r == 0x8000 && (q & 1)));
}

struct Axis {
  int o, te;  // tile origin in the square, outputs of the tile
  int ra, na; // A: first square index, count (F starts 6 before)
};
__device__ __forceinline__ Axis axis(int tile, int T, int n) {
  Axis x;
  x.o = tile * T;
  x.te = min(T, n - x.o);
  int lo, hi;
  refl_span(x.o - 13, x.o + x.te + 12, n, lo, hi);
  x.ra = lo, x.na = hi - lo + 1;
  return x;
}

}  // namespace

// DIR 0: Sobel(0,2) (d vertical, s horizontal), DIR 1: Sobel(2,0).  CV4: B rounds half up (GaussianBlurFixedPoint),
// else half to even (sepFilter2D's SIMD column pass).
template <int T, int DIR, bool CV4>
__global__ __launch_bounds__(kSB) void k_score_filter(const ScoreArgs a) {
  constexpr int PF = T + 38;  // F: (T + 38)^2 bytes at most
  constexpr int PH = T + 26;  // H: F rows x A cols (u16)
  constexpr int PA = T + 26;  // A: bytes
  constexpr int PP = T + 22;  // P: A rows x M cols (i16)
  constexpr int PM = T + 20;  // M: bytes, 0/1
  constexpr int PQ = T + 2;   // Q: M rows x tile cols (u16)
  constexpr int kBytes = PF * PF;
  constexpr int kHalves = (T + 38) * PH;
  static_assert(kBytes >= PA * PA && kBytes >= PM * PM, "byte buffer");
  static_assert(kHalves >= (T + 26) * PP && kHalves >= (T + 20) * PQ, "16-bit buffer");
  __shared__ uint8_t buf8[kBytes];
  __shared__ uint16_t buf16[kHalves];

  const int tiles = a.tiles;
  uint32_t b = blockIdx.x;
  const uint32_t f = b / uint32_t(tiles * tiles);
  b -= f * uint32_t(tiles * tiles);
  const int ty = int(b / uint32_t(tiles)), tx = int(b - uint32_t(ty) * uint32_t(tiles));
  const int n = a.n;
  const Axis X = axis(tx, T, n), Y = axis(ty, T, n);
  const uint8_t *src = a.src + f * a.src_frame_stride;

  // 1. F: frame rows y0 + Y.ra - 6 .. , columns x0 + X.ra - 6 .. (reflect101 about the FRAME)
  const int nfr = Y.na + 12, nfc = X.na + 12;  // nfc <= T + 38 <= 128
  {
    const int c = int(threadIdx.x & 127u);
    const uint32_t fc = uint32_t(refl(a.x0 + X.ra - 6 + c, a.width));
    if (c < nfc)
      for (int r = int(threadIdx.x >> 7); r < nfr; r += kSB / 128)
        buf8[r * PF + c] = src[uint32_t(refl(a.y0 + Y.ra - 6 + r, a.height)) * a.src_pitch + fc];
  }
  __syncthreads();
  // 2. H = G13 along rows: H[fr][ac] = sum_u t13[u] F[fr][ac + u]
  pass<6>(nfr, X.na, [&](int j) { return a.t13[j]; }, [&](int l, int i) { return int(buf8[l * PF + i]); },
          [&](int l, int o, int s) { buf16[l * PH + o] = uint16_t(s); });
  __syncthreads();
  // 3. A = rint_even(G13 along columns / 65536)
  pass<6>(X.na, Y.na, [&](int j) { return a.t13[j]; }, [&](int l, int i) { return int(buf16[i * PH + l]); },
          [&](int l, int o, int s) { buf8[o * PA + l] = uint8_t(round_even16(s)); });
  __syncthreads();
  // 4. Sobel along rows on the virtual M columns X.o - 10 + m (input i <-> virtual X.o - 13 + i)
  const int lmr = Y.te + 20, lmc = X.te + 20;
  auto s7 = [](int j) { return j == 3 ? 20 : (j == 2 || j == 4) ? 15 : (j == 1 || j == 5) ? 6 : 1; };
  auto d7 = [](int j) { return j == 3 ? -4 : (j == 2 || j == 4) ? -1 : (j == 1 || j == 5) ? 2 : 1; };
  pass<3>(Y.na, lmc, [&](int j) { return DIR == 0 ? s7(j) : d7(j); },
          [&](int l, int i) { return int(buf8[l * PA + refl(X.o - 13 + i, n) - X.ra]); },
          [&](int l, int o, int s) { buf16[l * PP + o] = uint16_t(int16_t(s)); });
  __syncthreads();
  // 5. ... along columns; threshold (0.03 I rounds above 30 exactly when I >= 1017)
  pass<3>(lmc, lmr, [&](int j) { return DIR == 0 ? d7(j) : s7(j); },
          [&](int l, int i) { return int(int16_t(buf16[(refl(Y.o - 13 + i, n) - Y.ra) * PP + l])); },
          [&](int l, int o, int s) { buf8[o * PM + l] = uint8_t(s >= 1017); });
  __syncthreads();
  // 6. Q = G21 of M along rows (M column i <-> virtual X.o - 10 + i)
  pass<10>(lmr, X.te, [&](int j) { return a.t21[j]; }, [&](int l, int i) { return int(buf8[l * PM + i]); },
           [&](int l, int o, int s) { buf16[l * PQ + o] = uint16_t(s); });
  __syncthreads();
  // 7. B = round(255 * G21 along columns / 65536); out = min(255, S + 2 B)
  uint8_t *out = a.out + f * a.out_frame_stride;
  uint8_t *grad = a.grad ? a.grad + f * a.grad_frame_stride : nullptr;
  const uint8_t *sq = src + uint32_t(a.y0 + Y.o) * a.src_pitch + uint32_t(a.x0 + X.o);
  pass<10>(X.te, Y.te, [&](int j) { return a.t21[j]; }, [&](int l, int i) { return int(buf16[i * PQ + l]); },
           [&](int l, int o, int s) {
             const int v = 255 * s;
             const int B = CV4 ? (v + 0x8000) >> 16 : round_even16(v);
             const int S = sq[uint32_t(o) * a.src_pitch + uint32_t(l)];
             out[uint32_t(Y.o + o) * a.out_pitch + uint32_t(X.o + l)] = uint8_t(min(255, S + 2 * B));
             if (grad) grad[uint32_t(Y.o + o) * a.grad_pitch + uint32_t(X.o + l)] = uint8_t(B);
           });
}

namespace {

// DESIGN.md section 8a.  G13: OpenCV's general 8-bit path rounds the float kernel to 1/256 units (both
// generations).  G21, CV4: ufixedpoint16 taps by error-diffused rounding from the outside in, the centre takes the
// remainder (sum 256).  G21, CV3: OpenCV 3.2's getGaussianKernel (float taps, double sum), then the general path.
void gauss_bitexact(int n, double sigma, double *g) {  // getGaussianKernelBitExact (4.x)
  const double scale2 = -0.125 / (sigma * sigma);
  double sum = 0;
  for (int i = 0, x = 1 - n; i < n / 2; ++i, x += 2) g[i] = std::exp(double(x * x) * scale2), sum += g[i];
  sum = sum * 2 + 1;
  const double mul = 1 / sum;
  for (int i = 0; i < n / 2; ++i) g[i] = g[n - 1 - i] = g[i] * mul;
  g[n / 2] = mul;
}
void gauss_cv3(int n, double sigma, double *g) {  // getGaussianKernel(n, sigma, CV_32F) of OpenCV 3.2
  const double scale2 = -0.5 / (sigma * sigma);
  float cf[32];
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    cf[i] = float(std::exp(scale2 * x * x));
    sum += cf[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < n; ++i) g[i] = double(float(cf[i] * sum));
}
void general_taps(int n, const double *g, int32_t *t) {  // convertTo(CV_32S, 256): cvRound of the float value
  for (int i = 0; i < n; ++i) t[i] = int32_t(std::nearbyint(double(float(g[i])) * 256.0));
}
void fixed_point_taps(int n, const double *g, int32_t *t) {  // getGaussianKernelFixedPoint_ED, 8 fraction bits
  double err = 0;
  int32_t sum = 0;
  for (int i = 0; i < n / 2; ++i) {
    const double adj = g[i] * 256.0 + err;
    const int32_t v = int32_t(std::nearbyint(adj));
    err = adj - v;
    t[i] = t[n - 1 - i] = v;
    sum += v;
  }
  t[n / 2] = 256 - 2 * sum;
}

template <int T>
hipError_t launch_tile(const ScoreArgs &a, hipStream_t stream) {
  const uint64_t blocks = uint64_t(a.tiles) * a.tiles * a.n_frames;
  if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid{uint32_t(blocks), 1, 1}, block{kSB, 1, 1};
  const bool cv4 = a.form == 4;
  if (a.direction == 0 && cv4)
    hipLaunchKernelGGL((k_score_filter<T, 0, true>), grid, block, 0, stream, a);
  else if (a.direction == 0)
    hipLaunchKernelGGL((k_score_filter<T, 0, false>), grid, block, 0, stream, a);
  else if (cv4)
    hipLaunchKernelGGL((k_score_filter<T, 1, true>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((k_score_filter<T, 1, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_score_filter(ScoreArgs a, hipStream_t stream) {
  if (a.n < 11 || (a.direction != 0 && a.direction != 1) || (a.form != 3 && a.form != 4)) return hipErrorInvalidValue;
  double g[21];
  gauss_bitexact(13, 3.0, g);
  general_taps(13, g, a.t13);
  if (a.form == 4) {
    gauss_bitexact(21, 10.0, g);
    fixed_point_taps(21, g, a.t21);
  } else {
    gauss_cv3(21, 10.0, g);
    general_taps(21, g, a.t21);
  }
  // 64 x 64 tiles (halo recompute x2 in A); 32 x 32 when that leaves most CUs idle (one 465 x 465 frame)
  const int t64 = (a.n + 63) / 64;
  if (a.tile != 0 && a.tile != 32 && a.tile != 64) return hipErrorInvalidValue;
  if (a.tile ? a.tile == 64 : uint64_t(t64) * t64 * a.n_frames >= 512) {
    a.tiles = t64;
    return launch_tile<64>(a, stream);
  }
  a.tiles = (a.n + 31) / 32;
  return launch_tile<32>(a, stream);
}

}  // namespace d2pc
