// d2pc_colorize.hip -- colorizeDepth of the depth_map_fusion node on gfx950 (reference src/depth_map_fusion.cpp:306-360)
// fused with what precedes it in DisparityCb1/2 (:45-61): the view cropToSquare takes, of the frame or of the frame
// rotated 90 degrees clockwise (rotateMat), never materialising the rotated frame.
//
// The colouring is a function of the 8-bit pixel alone: a 256 x 3 table, computed on the HOST in IEEE float32
// (colorize_table below) and handed to the kernel as launch data.  The device evaluates no
// float expression; the kernel moves 1 byte in and 1 + 3 bytes out per pixel and is a memory kernel.
//
// A workgroup owns a 128 x 64 tile of the view.
//  * In: the tile is staged in LDS in VIEW orientation, 33 dwords per row (32 + 1 pad).  Unrotated, a wave
//    instruction loads two 128-byte row pieces.  Rotated, the tile is 128 source rows of 64 bytes: a thread loads the
//    same dword column of four adjacent source rows, transposes the 4 x 4 byte block in registers (two v_perm
//    levels, as k_rotate_cw does) and writes four dwords; the pad keeps those column writes at two per bank.
//  * Out: the unit of work is an ALIGNED piece of an output row -- 12 bytes of rgb (three dwords, one store
//    instruction) and 4 bytes of gray -- whatever the row's base address is: unit k of a row covers the bytes
//    [12 k - a, 12 k - a + 12) of the tile's rgb row, a = its address & 3, which are the pixels 4k-1 .. 4k+3 (or
//    4k .. 4k+3 when a = 0) from channel 3 - a on.  The five table dwords are spliced with byte alignments
//    (v_alignbyte).  Only the first and last unit of a tile row, where the 12 bytes stick out of the tile, fall back
//    to byte stores; 33 units cover a 128-pixel row for every a.  Consecutive lanes take consecutive units, so a wave
//    stores 768 contiguous bytes of rgb.
//  * The table sits in LDS as one dword per entry; the lookups are data-dependent ds_read_b32 (up to five per 12
//    output bytes), whose bank conflicts are the price of a table at all (equal neighbours broadcast).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "d2pc_launch.hpp"

namespace d2pc {

namespace {

constexpr int kTW = 128, kTH = 64;     // tile of the view: columns, rows
constexpr int kRow = kTW / 4 + 1;      // dwords per staged row (one pad)
constexpr int kUnits = kTW / 4 + 1;    // aligned output units per tile row: (3 * 128 + 3) / 12 < 33
constexpr int kCB = 256;               // threads per workgroup

// Bytes p[0 .. valid) of a dword (1 <= valid <= 3): the last, partial dword of a tile row.
__device__ __forceinline__ uint32_t load_partial(const uint8_t *p, int valid) {
  uint32_t v = p[0];
  if (valid > 1) v |= uint32_t(p[1]) << 8;
  if (valid > 2) v |= uint32_t(p[2]) << 16;
  return v;
}

// o[i] = (byte i of b0, of b1, of b2, of b3), lowest address first
__device__ __forceinline__ void transpose_4x4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t (&o)[4]) {
  const uint32_t a0 = __builtin_amdgcn_perm(b1, b0, 0x05010400u), a1 = __builtin_amdgcn_perm(b1, b0, 0x07030602u);
  const uint32_t a2 = __builtin_amdgcn_perm(b3, b2, 0x05010400u), a3 = __builtin_amdgcn_perm(b3, b2, 0x07030602u);
  o[0] = __builtin_amdgcn_perm(a2, a0, 0x05040100u);
  o[1] = __builtin_amdgcn_perm(a2, a0, 0x07060302u);
  o[2] = __builtin_amdgcn_perm(a3, a1, 0x05040100u);
  o[3] = __builtin_amdgcn_perm(a3, a1, 0x07060302u);
}

struct Dword3 {
  uint32_t v[3];
};

}  // namespace

template <bool ROT>
__global__ __launch_bounds__(kCB) void k_colorize(const ColorizeArgs a) {
  __shared__ uint32_t tile[kTH * kRow];
  __shared__ uint32_t lut[256];
  const int t = int(threadIdx.x);
  lut[t] = a.table[t];

  uint32_t b = blockIdx.x;
  const uint32_t per_frame = a.tiles_x * a.tiles_y;
  const uint32_t f = b / per_frame;
  b -= f * per_frame;
  const uint32_t tyi = b / a.tiles_x, txi = b - tyi * a.tiles_x;
  const int tx0 = int(txi) * kTW, ty0 = int(tyi) * kTH;  // tile origin in the view
  const int tw = min(kTW, a.w - tx0), th = min(kTH, a.h - ty0);
  const uint8_t *src = a.src + uint64_t(f) * a.src_frame_stride;

  if (!ROT) {
    // view (vx, vy) = src(a.y + ty0 + vy, a.x + tx0 + vx): thread (r, c) takes dword c of the rows r, r + 8, ...
    // Rows past the tile's end repeat its last row (branch-free loads, all in flight together; nobody reads them).
    const int c = t & 31, r = t >> 5;
    const int valid = tw - 4 * c;
    if (valid > 0) {
      const uint8_t *p = src + uint64_t(a.y + ty0) * a.src_pitch + uint32_t(a.x + tx0 + 4 * c);
      uint32_t v[kTH / 8];
      if (valid >= 4) {
#pragma unroll
        for (int k = 0; k < kTH / 8; ++k) __builtin_memcpy(&v[k], p + uint64_t(min(r + 8 * k, th - 1)) * a.src_pitch, 4);
      } else {
#pragma unroll
        for (int k = 0; k < kTH / 8; ++k) v[k] = load_partial(p + uint64_t(min(r + 8 * k, th - 1)) * a.src_pitch, valid);
      }
#pragma unroll
      for (int k = 0; k < kTH / 8; ++k) tile[(r + 8 * k) * kRow + c] = v[k];
    }
  } else {
    // view (vx, vy) = src(rows - 1 - (a.x + tx0 + vx), a.y + ty0 + vy): the tile is 128 source rows of 64 bytes.
    // Thread (g, c): dword column c (vy = 4c .. 4c+3) of the four source rows of vx = 4g .. 4g+3.
    // Columns past the tile's end repeat its last column.
    const int c = t & 15;
    const int valid = th - 4 * c;
    if (valid > 0) {
      uint32_t blk[kTW / 64][4];
      auto at = [&](int it, int k) {  // source row of vx = 4g + k
        const int vx = min(4 * ((t >> 4) + 16 * it) + k, tw - 1);
        return src + uint64_t(a.rows - 1 - (a.x + tx0 + vx)) * a.src_pitch + uint32_t(a.y + ty0 + 4 * c);
      };
      if (valid >= 4) {
#pragma unroll
        for (int i = 0; i < kTW / 16; ++i) __builtin_memcpy(&blk[i >> 2][i & 3], at(i >> 2, i & 3), 4);
      } else {
#pragma unroll
        for (int i = 0; i < kTW / 16; ++i) blk[i >> 2][i & 3] = load_partial(at(i >> 2, i & 3), valid);
      }
#pragma unroll
      for (int it = 0; it < kTW / 64; ++it) {
        const int g = (t >> 4) + 16 * it;
        uint32_t o[4];
        transpose_4x4(blk[it][0], blk[it][1], blk[it][2], blk[it][3], o);
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[(4 * c + i) * kRow + g] = o[i];
      }
    }
  }
  __syncthreads();

  uint8_t *gray = a.gray ? a.gray + uint64_t(f) * a.gray_frame_stride + uint64_t(ty0) * a.gray_pitch + uint32_t(tx0) : nullptr;
  uint8_t *rgb = a.rgb ? a.rgb + uint64_t(f) * a.rgb_frame_stride + uint64_t(ty0) * a.rgb_pitch + 3u * uint32_t(tx0) : nullptr;
  const int items = th * kUnits;
  for (int it = t; it < items; it += kCB) {
    const int vy = it / kUnits, k = it - vy * kUnits;
    // the pixels 4k-4 .. 4k-1 and 4k .. 4k+3 of the tile row (k = 32 reads the pad: every use of it is masked)
    const uint32_t lo = tile[vy * kRow + max(k - 1, 0)], hi = tile[vy * kRow + k];
    if (gray) {  // launch-uniform
      uint8_t *row = gray + uint64_t(vy) * a.gray_pitch;
      const int al = int(reinterpret_cast<uintptr_t>(row) & 3u);
      const int first = 4 * k - al;  // tile column of the unit's first byte
      const uint32_t v = al ? __builtin_amdgcn_alignbyte(hi, lo, uint32_t(4 - al)) : hi;
      if (first >= 0 && first + 4 <= tw) {
        *reinterpret_cast<uint32_t *>(row + first) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (first + j >= 0 && first + j < tw) row[first + j] = uint8_t(v >> (8 * j));
      }
    }
    if (rgb) {  // launch-uniform
      uint8_t *row = rgb + uint64_t(vy) * a.rgb_pitch;
      const int al = int(reinterpret_cast<uintptr_t>(row) & 3u);
      const int first = 12 * k - al;  // byte of the tile's rgb row the unit starts at
      if (first < 3 * tw) {
        // the unit's pixels: 4k-1 .. 4k+3 from channel 3 - al on (al = 0: 4k .. 4k+3 from channel 0)
        const uint32_t px = al ? __builtin_amdgcn_alignbyte(hi, lo, 3u) : hi;
        const uint32_t t0 = lut[px & 255u], t1 = lut[(px >> 8) & 255u], t2 = lut[(px >> 16) & 255u], t3 = lut[px >> 24];
        const uint32_t t4 = al ? lut[hi >> 24] : 0u;
        // the 15 table bytes as a stream of dwords, then shifted to the unit's first byte
        const uint32_t s0 = t0 | (t1 << 24), s1 = (t1 >> 8) | (t2 << 16), s2 = (t2 >> 16) | (t3 << 8), s3 = t4;
        const uint32_t sh = al ? uint32_t(3 - al) : 0u;
        Dword3 o;
        o.v[0] = __builtin_amdgcn_alignbyte(s1, s0, sh);
        o.v[1] = __builtin_amdgcn_alignbyte(s2, s1, sh);
        o.v[2] = __builtin_amdgcn_alignbyte(s3, s2, sh);
        if (first >= 0 && first + 12 <= 3 * tw) {
          *reinterpret_cast<Dword3 *>(row + first) = o;
        } else {
#pragma unroll
          for (int j = 0; j < 12; ++j)
            if (first + j >= 0 && first + j < 3 * tw) row[first + j] = uint8_t(o.v[j >> 2] >> (8 * (j & 3)));
        }
      }
    }
  }
}

// colorizeDepth per 8-bit value.  Every float operation is one IEEE float32 operation in the
// order the reference writes it: no contraction, no reassociation, no reciprocal in place of the division.
#pragma clang fp contract(off) reassociate(off)
void colorize_table(uint8_t table[768]) {
#pragma clang fp contract(off) reassociate(off)
  for (int g = 0; g < 256; ++g) {
    const unsigned char d = static_cast<unsigned char>(40 + 0.8 * g);  // double; = 40 + 4 g / 5
    const unsigned int H = 255u - (255u - d) * 280u / 255u;             // 19 .. 243
    const unsigned int hi = (H / 60u) % 6u;                             // 0 .. 4
    volatile float quo = float(H) / 60.f;   // volatile: each result is rounded to float32 and stored
    volatile float f = quo - float(H / 60u);
    volatile float q = 1.f - f;
    volatile float u = 1.f - f;
    volatile float tt = 1.f - u;
    const float p = 0.f, V = 1.f;
    float x = 0.f, y = 0.f, z = 0.f;
    switch (hi) {
      case 0: x = p, y = tt, z = V; break;
      case 1: x = p, y = V, z = q; break;
      case 2: x = tt, y = V, z = p; break;
      case 3: x = V, y = q, z = p; break;
      case 4: x = V, y = p, z = tt; break;
      default: x = q, y = p, z = V; break;  // unreachable: H <= 243
    }
    auto byte = [](float v) {
      volatile float s = std::max(0.f, std::min(v, 1.f)) * 255.f;
      return static_cast<unsigned char>(s);  // truncation
    };
    uint8_t *row = table + 3 * g;
    row[0] = byte(x), row[1] = byte(y), row[2] = byte(z);
    if (d == 40) row[0] = row[1] = row[2] = 0;  // g = 0 and g = 1
  }
}

hipError_t launch_colorize(ColorizeArgs a, hipStream_t stream) {
  if (a.w <= 0 || a.h <= 0 || a.n_frames <= 0 || (!a.gray && !a.rgb)) return hipErrorInvalidValue;
  a.tiles_x = uint32_t((a.w + kTW - 1) / kTW);
  a.tiles_y = uint32_t((a.h + kTH - 1) / kTH);
  const uint64_t blocks = uint64_t(a.tiles_x) * a.tiles_y * uint32_t(a.n_frames);
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  static const struct Table {
    uint32_t e[256];
    Table() {
      uint8_t t[768];
      colorize_table(t);
      for (int g = 0; g < 256; ++g) e[g] = uint32_t(t[3 * g]) | (uint32_t(t[3 * g + 1]) << 8) | (uint32_t(t[3 * g + 2]) << 16);
    }
  } table;
  for (int g = 0; g < 256; ++g) a.table[g] = table.e[g];
  const dim3 grid{uint32_t(blocks), 1, 1}, block{kCB, 1, 1};
  if (a.rotate_cw)
    hipLaunchKernelGGL(k_colorize<true>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(k_colorize<false>, grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace d2pc
