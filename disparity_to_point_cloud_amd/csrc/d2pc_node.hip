// d2pc_node.hip -- the fusing DisparityCb2 of the depth_map_fusion node in ONE launch on gfx950 (reference
// src/depth_map_fusion.cpp:53-61 and publishFusedDepthMap :102-135).  The three-launch
// composition (k_colorize<true>, k_fuse_median3, k_colorize<false>) is launch-bound at the reference geometry: a
// 465 x 465 square is 32 workgroups of each of them.  This kernel does the whole body per TILE of the square:
//
//   A  stage the tile with a one-pixel halo in LDS: camera 1's depth and the two score planes as they are, camera 2's
//      depth straight from its RAW frame through the rotated, cropped view (view (vx, vy) = frame(rows - 1 - (x2 + vx),
//      y2 + vy); the rotated frame is never materialised, the gray plane of camera 2 never stored: nothing reads it
//      after a fusing callback).  Load coordinates are clamped to the square, which replicates the borders for the
//      median (the rule is per pixel, so that equals replicating the fused image).
//   B  per dword of four pixels: GRAD_FILTER on pairs (fuse_pair of d2pc_fuse_pair.hpp) -> the fused tile with its halo
//      in LDS; for the tile's own pixels also min(grad1, grad2) -> the spare plane, and the colouring of camera 2's
//      depth -> /cropped_depth_2.
//   C  3 x 3 median of the fused tile from sorted vertical triples (two pixels per instruction), crop, then the fused
//      map and its colouring through the 256-entry table in LDS.
//
// A tile is 64 columns by 16 rows (240 workgroups for the 465 x 465 square: one frame fills the machine) or by 64 rows
// (large batches: a quarter of the halo rows, and 66-byte runs of the raw frame per view column instead of 18).
// Reads: raw frame, depth 1, score 1, score 2.  Writes: spare, two colour images, fused map.  No output aliases an
// input (the score1 <-> spare swap is host state of the session, done after the launch is enqueued).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "d2pc_launch.hpp"
#include "d2pc_fuse_pair.hpp"

namespace d2pc {

namespace {

constexpr int kNTW = 64;             // tile columns
constexpr int kNRowDw = 18;          // dwords per staged row: columns tx0 - 4 .. tx0 + 67, of which tx0 - 1 .. tx0 + 64 are loaded
constexpr int kNRowB = 4 * kNRowDw;  // ... in bytes; column tx0 - 1 + c sits at byte 3 + c, so the tile's own dwords are aligned
constexpr int kNBlock = 256;
constexpr uint32_t kSelE = 0x0c020c00u, kSelO = 0x0c030c01u;  // v_perm_b32: bytes (0, 2) / (1, 3) as two 16-bit fields

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// An n x n plane's tile with halo into LDS, coordinates clamped to the plane.
template <int R>
__device__ __forceinline__ void stage_plane(const uint8_t *__restrict__ plane, uint64_t pitch, int n, int tx0, int ty0,
                                            uint32_t *lds, int t) {
  uint8_t *ldsb = reinterpret_cast<uint8_t *>(lds);
  if (tx0 + kNTW <= n) {  // block-uniform: the tile's 64 columns as 16 dwords (any alignment), the two halo columns as bytes
    for (int i = t; i < R * kNRowDw; i += kNBlock) {
      const int r = i / kNRowDw, k = i - r * kNRowDw;
      const uint8_t *row = plane + uint64_t(clampi(ty0 - 1 + r, 0, n - 1)) * pitch;
      if (k < 16) {
        uint32_t v;
        __builtin_memcpy(&v, row + tx0 + 4 * k, 4);
        lds[r * kNRowDw + 1 + k] = v;
      } else if (k == 16) {
        ldsb[r * kNRowB + 3] = row[max(tx0 - 1, 0)];
      } else {
        ldsb[r * kNRowB + 4 + kNTW] = row[min(tx0 + kNTW, n - 1)];
      }
    }
  } else {
    for (int i = t; i < R * (kNTW + 2); i += kNBlock) {
      const int r = i / (kNTW + 2), c = i - r * (kNTW + 2);
      const uint8_t *row = plane + uint64_t(clampi(ty0 - 1 + r, 0, n - 1)) * pitch;
      ldsb[r * kNRowB + 3 + c] = row[clampi(tx0 - 1 + c, 0, n - 1)];
    }
  }
}

// The colouring of the pixels x .. x+3 (the bytes of px) whose column lies in [lo, hi), at row[3 (x - lo)].
__device__ __forceinline__ void store_rgb4(uint8_t *__restrict__ row, int x, int lo, int hi, uint32_t px, const uint32_t *lut) {
  const uint32_t c[4] = {lut[px & 255u], lut[(px >> 8) & 255u], lut[(px >> 16) & 255u], lut[px >> 24]};
  if (x >= lo && x + 3 < hi) {
    const uint32_t o[3] = {c[0] | (c[1] << 24), (c[1] >> 8) | (c[2] << 16), (c[2] >> 16) | (c[3] << 8)};
    __builtin_memcpy(row + 3 * (x - lo), o, 12);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (x + k >= lo && x + k < hi) {
      uint8_t *p = row + 3 * (x + k - lo);
      p[0] = uint8_t(c[k]), p[1] = uint8_t(c[k] >> 8), p[2] = uint8_t(c[k] >> 16);
    }
}

// median of nine on pairs: v[row][column]; sorted vertical triples, then med3(max of the lows, med of the mids, min of the highs)
__device__ __forceinline__ uint32_t pk_med9(const uint32_t (&v)[3][3]) {
  uint32_t lo[3], me[3], hi[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t mn = pk_min(v[0][c], v[1][c]), mx = pk_max(v[0][c], v[1][c]);
    lo[c] = pk_min(mn, v[2][c]);
    hi[c] = pk_max(mx, v[2][c]);
    me[c] = pk_max(mn, pk_min(mx, v[2][c]));
  }
  return pk_med3(pk_max(pk_max(lo[0], lo[1]), lo[2]), pk_med3(me[0], me[1], me[2]), pk_min(pk_min(hi[0], hi[1]), hi[2]));
}

}  // namespace

template <int TH>
__global__ __launch_bounds__(kNBlock) void k_node_fuse(const NodeFuseArgs a) {
  constexpr int R = TH + 2;
  __shared__ uint32_t pd1[R * kNRowDw], pd2[R * kNRowDw], ps1[R * kNRowDw], ps2[R * kNRowDw], pfu[R * kNRowDw];
  __shared__ uint32_t lut[256];
  const int t = int(threadIdx.x);
  lut[t] = a.table[t];

  uint32_t b = blockIdx.x;
  const uint32_t per_frame = a.tiles_x * a.tiles_y;
  const uint32_t f = b / per_frame;
  b -= f * per_frame;
  const uint32_t tyi = b / a.tiles_x, txi = b - tyi * a.tiles_x;
  const int n = a.n, tx0 = int(txi) * kNTW, ty0 = int(tyi) * TH;

  // ---- A: stage
  stage_plane<R>(a.depth1 + uint64_t(f) * a.depth1_frame_stride, a.depth1_pitch, n, tx0, ty0, pd1, t);
  stage_plane<R>(a.score1 + uint64_t(f) * a.score1_frame_stride, a.score1_pitch, n, tx0, ty0, ps1, t);
  stage_plane<R>(a.score2 + uint64_t(f) * a.score2_frame_stride, a.score2_pitch, n, tx0, ty0, ps2, t);
  {
    // consecutive threads walk DOWN a view column: those bytes are consecutive in the raw frame's row
    const uint8_t *src = a.frame2 + uint64_t(f) * a.frame2_frame_stride;
    uint8_t *ldsb = reinterpret_cast<uint8_t *>(pd2);
    for (int i = t; i < R * (kNTW + 2); i += kNBlock) {
      const int c = i / R, r = i - c * R;
      const int vx = clampi(tx0 - 1 + c, 0, n - 1), vy = clampi(ty0 - 1 + r, 0, n - 1);
      ldsb[r * kNRowB + 3 + c] = src[uint64_t(a.rows - 1 - (a.x2 + vx)) * a.frame2_pitch + uint32_t(a.y2 + vy)];
    }
  }
  __syncthreads();

  // ---- B: the rule on every staged dword; the tile's own pixels also give the combined plane and camera 2's colouring
  uint8_t *spare = a.spare + uint64_t(f) * a.spare_frame_stride;
  uint8_t *rgb2 = a.rgb2 + uint64_t(f) * a.rgb2_frame_stride;
  for (int i = t; i < R * kNRowDw; i += kNBlock) {
    const int r = i / kNRowDw, k = i - r * kNRowDw;
    const uint32_t d1 = pd1[i], d2 = pd2[i], s1 = ps1[i], s2 = ps2[i];
    const uint32_t s1e = __builtin_amdgcn_perm(s1, s1, kSelE), s2e = __builtin_amdgcn_perm(s2, s2, kSelE);
    const uint32_t s1o = __builtin_amdgcn_perm(s1, s1, kSelO), s2o = __builtin_amdgcn_perm(s2, s2, kSelO);
    const uint32_t fe = fuse_pair<FUSE_GRAD_FILTER>(__builtin_amdgcn_perm(d1, d1, kSelE), __builtin_amdgcn_perm(d2, d2, kSelE), s1e, s2e);
    const uint32_t fo = fuse_pair<FUSE_GRAD_FILTER>(__builtin_amdgcn_perm(d1, d1, kSelO), __builtin_amdgcn_perm(d2, d2, kSelO), s1o, s2o);
    pfu[i] = fe | (fo << 8);
    const int y = ty0 + r - 1, x = tx0 + 4 * (k - 1);
    if (r >= 1 && r <= TH && k >= 1 && k <= 16 && y < n && x < n) {
      store_px4(spare + uint64_t(y) * a.spare_pitch, x, 0, n, pk_min(s1e, s2e) | (pk_min(s1o, s2o) << 8));  // (:118-121)
      store_rgb4(rgb2 + uint64_t(y) * a.rgb2_pitch, x, 0, n, d2, lut);
    }
  }
  __syncthreads();

  // ---- C: median, crop, the fused map and its colouring
  uint8_t *fused = a.fused + uint64_t(f) * a.fused_frame_stride;
  uint8_t *grad = a.gradient + uint64_t(f) * a.gradient_frame_stride;
  const int cx0 = a.crop_left, cx1 = cx0 + a.out_width, cy0 = a.crop_top, cy1 = cy0 + a.out_height;
  for (int i = t; i < TH * 16; i += kNBlock) {
    const int r = i >> 4, k = i & 15;
    const int y = ty0 + r, x = tx0 + 4 * k;
    if (y < cy0 || y >= cy1 || x + 3 < cx0 || x >= cx1) continue;  // (cx1, cy1 <= n)
    uint32_t e[3][3], o[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {  // staged rows r .. r + 2 are the image rows y - 1 .. y + 1
      const uint32_t *row = pfu + (r + j) * kNRowDw + k;
      const uint32_t prev = row[0], cur = row[1], next = row[2];
      const uint32_t col[3] = {__builtin_amdgcn_alignbyte(cur, prev, 3u), cur, __builtin_amdgcn_alignbyte(next, cur, 1u)};
#pragma unroll
      for (int c = 0; c < 3; ++c) {  // columns x-1 .. x+2, x .. x+3, x+1 .. x+4
        e[j][c] = __builtin_amdgcn_perm(col[c], col[c], kSelE);
        o[j][c] = __builtin_amdgcn_perm(col[c], col[c], kSelO);
      }
    }
    const uint32_t m = pk_med9(e) | (pk_med9(o) << 8);
    store_px4(fused + uint64_t(y - cy0) * a.fused_pitch, x, cx0, cx1, m);
    store_rgb4(grad + uint64_t(y - cy0) * a.gradient_pitch, x, cx0, cx1, m, lut);
  }
}

hipError_t launch_node_fuse(NodeFuseArgs a, hipStream_t stream, int tile_rows) {
  if (a.n <= 0 || a.n_frames <= 0 || a.out_width <= 0 || a.out_height <= 0 || !a.table) return hipErrorInvalidValue;
  a.tiles_x = uint32_t((a.n + kNTW - 1) / kNTW);
  const uint64_t tall = uint64_t(a.tiles_x) * uint32_t((a.n + 63) / 64) * uint32_t(a.n_frames);
  const int th = (tile_rows == 16 || tile_rows == 64) ? tile_rows : (tall >= 2048u ? 64 : 16);
  a.tiles_y = uint32_t((a.n + th - 1) / th);
  const uint64_t blocks = uint64_t(a.tiles_x) * a.tiles_y * uint32_t(a.n_frames);
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid{uint32_t(blocks), 1, 1}, block{kNBlock, 1, 1};
  if (th == 64)
    hipLaunchKernelGGL(k_node_fuse<64>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(k_node_fuse<16>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace d2pc
