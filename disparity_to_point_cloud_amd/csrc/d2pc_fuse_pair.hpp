// d2pc_fuse_pair.hpp -- the fusion rules on PAIRS of pixels (two 16-bit fields per dword), shared by the kernels that
// fuse: k_fuse_median3 (d2pc_fusion.hip) and the single-launch DisparityCb2 of the node session (d2pc_node.hip).
// Device code only; include after <hip/hip_runtime.h> and d2pc_launch.hpp (the FUSE_* rule numbers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "d2pc_launch.hpp"

namespace d2pc {

namespace {

// ---- two 16-bit fields per dword -------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk(uint32_t c) { return c | (c << 16); }  // both fields = c
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {         // per-field a - b (wraps)
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {         // per-field a + b (wraps)
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pk_shl2(uint32_t a) {                    // per-field a << 2
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) << 2);
}
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
// field mask (0xffff / 0) from the sign bit of each field.  Inline asm: written
// as a vector shift, LLVM turns mask-and-pick into per-field compare + select,
// which has no packed form and costs five instructions instead of one.
__device__ __forceinline__ uint32_t pk_sign_mask(uint32_t a) {
  uint32_t r;
  asm("v_pk_ashrrev_i16 %0, 15, %1 op_sel_hi:[0,1]" : "=v"(r) : "v"(a));
  return r;
}
__device__ __forceinline__ uint32_t pk_half(uint32_t a) {  // per-field a >> 1
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) >> 1);
}
__device__ __forceinline__ uint32_t pick(uint32_t mask, uint32_t a, uint32_t b) { return (a & mask) | (b & ~mask); }
__device__ __forceinline__ uint32_t pk_med3(uint32_t a, uint32_t b, uint32_t c) {
  return pk_max(pk_min(a, b), pk_min(pk_max(a, b), c));
}

// The selected rule (reference src/depth_map_fusion.cpp:162-235) on a pair of
// pixels; every operand field holds an 8-bit value.  lt(a, b) below is "the
// sign bit of a - b", valid while |a - b| < 2^15.
// GRAD_FILTER's float test 0.8 < float(d1)/float(d2) < 1.25 (cpp:224,230) is
// 5*d1 >= 4*d2 && 4*d1 < 5*d2: the quotient is compared as a float against
// DOUBLE literals, float(0.8) > 0.8 so the exact ratio 4/5 passes, 5/4 is exact
// and fails, no other 8-bit ratio is within a float ulp of either bound, and
// d2 == 0 (inf or NaN) fails both ways.
template <int RULE>
__device__ __forceinline__ uint32_t fuse_pair(uint32_t d1, uint32_t d2, uint32_t s1, uint32_t s2) {
  const uint32_t avg = pk_half(d1 + d2);
  switch (RULE) {
    case FUSE_WEIGHTED_AVERAGE: {  // int weights: 1 for score 0, else 0; 0/0 (undefined there) -> 0
      const uint32_t w1 = pk_sign_mask(pk_sub(s1, pk(1))), w2 = pk_sign_mask(pk_sub(s2, pk(1)));
      return pick(w1, pick(w2, avg, d1), w2 & d2);
    }
    case FUSE_MAX_DIST: return pk_min(d1, d2);
    case FUSE_MAX_DIST_UNLESS_BLACK: {
      const uint32_t black = pk_sign_mask(pk_sub(d1, pk(1)) | pk_sub(d2, pk(1)));
      return pick(black, pk_max(d1, d2), pk_min(d1, d2));
    }
    case FUSE_BETTER_SCORE: return pick(pk_sign_mask(pk_sub(s1, s2)), d1, d2);
    case FUSE_ONLY_GOOD_1: return pk_sign_mask(pk_sub(s2, pk(50))) & d2;
    case FUSE_ONLY_GOOD_AVG: return pk_sign_mask(pk_sub(s1, pk(100)) & pk_sub(s2, pk(100))) & avg;
    case FUSE_OVERLAP: {
      const uint32_t a = pk_sign_mask(pk_sub(s1, s2) & pk_sub(s1, pk(20)));
      const uint32_t b = pk_sign_mask(pk_sub(s2, s1) & pk_sub(s2, pk(20)));
      return pick(a, pk(150), b & pk(255));
    }
    case FUSE_BLACK_TO_WHITE: return pk(255) - s1;
    default: {  // FUSE_GRAD_FILTER
      const uint32_t a = pk_sign_mask(pk_sub(s1, s2) & pk_sub(s1, pk(100)) & pk_sub(d1, pk(230)));
      const uint32_t b = pk_sign_mask(pk_sub(s2, s1) & pk_sub(s2, pk(100)) & pk_sub(d2, pk(230)));
      // 5*d1 >= 4*d2 && 4*d1 < 5*d2  <=>  t + d1 >= 0 && t - d2 < 0  with  t = 4*(d1 - d2)
      const uint32_t t = pk_shl2(pk_sub(d1, d2));
      const uint32_t c = pk_sign_mask(~pk_add(t, d1) & pk_sub(t, d2) & pk_sub(s1, pk(125)) & pk_sub(s2, pk(125)));
      return pick(a, d1, pick(b, d2, c & avg));
    }
  }
}

// Stores the bytes of v whose column lies in [lo, hi) at dst[x - lo].
__device__ __forceinline__ void store_px4(uint8_t *__restrict__ dst_row, int x, int lo, int hi, uint32_t v) {
  if (x >= lo && x + 3 < hi) {
    __builtin_memcpy(dst_row + (x - lo), &v, 4);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (x + k >= lo && x + k < hi) dst_row[x + k - lo] = uint8_t(v >> (8 * k));
}

}  // namespace

}  // namespace d2pc
