// d2pc_rig.hip -- the rig session's kernels: N cameras of one geometry, each with its own Q (a pose folded in as T.Q),
// into ONE cloud.  PARITY: camera f's ROI points at point f * roi_n, reference order (cpp:70-76).  COMPACT: the
// survivors of camera 0, then of camera 1, ..., dense; count per tile -> one scan over all tiles of all cameras ->
// scatter, three launches and no block waiting on another.  The scatter recomputes the points the count looked at.
//
// A block works on one tile of ONE camera (blockIdx.y): its calibration is a wave-uniform entry of a small table in
// device memory, read through scalar loads, and the arithmetic -- the reproject() overloads of d2pc_pixel.hpp, none
// restated here -- is chosen by a wave-uniform branch on (stereoRectify structure, form).  Kernels are templated on the
// input dtype only.  A point's position in the merged cloud is a 32-bit number (the host refuses n * roi_n >= 2^32);
// its address is formed in 64 bits: the cloud may exceed 4 GiB.
//
// Also here, to share this code object: k_texture, the gather behind d2pc_texture_device (any producer's points + a
// per-pixel plane -> 32-byte PointXYZI / PointXYZRGB records).
#include "d2pc_compact_common.hpp"
#include "d2pc_rig.hpp"

namespace d2pc {

// f(QArg) with the camera's Q in the kind fill_q would choose for it (d2pc_capi_context.hip; never OpenCV 2.4's form)
template <class F>
__device__ __forceinline__ void with_camera_q(const RigCal &e, uint32_t cv4, F &&f) {
  if (e.stereo) {
    if (!cv4) {
      QArg<QK_STEREO> A;
      A.s = QStereo{e.cx, e.cy, e.f, e.a, e.b, 0.0};
      f(A);
    } else {
      QArg<QK_STEREO_CV4> A;
      A.s = QStereo{e.cx, e.cy, e.f_cv4, e.a, e.b, 0.0};
      f(A);
    }
  } else {
    QArg<QK_GENERAL> A;
#pragma unroll
    for (int i = 0; i < 16; ++i) A.m.q[i] = e.q[i];
    A.m.form = 0u;  // OpenCV 3/4's association: the default for a dense Q, and D2PC_FORM_CV4
    f(A);
  }
}

// Disparities and image coordinates of a thread's S pixels: pixel k is ROI pixel lt * 256 * S + k * 256 + thread.
template <int DT, int S>
__device__ __forceinline__ void rig_load(float (&d)[S], uint32_t (&uu)[S], uint32_t (&vv)[S], const uint8_t *fin, const Geom &g,
                                         uint32_t base) {
#pragma unroll
  for (int k = 0; k < S; ++k) {
    pixel_coords(g, base + uint32_t(k) * uint32_t(kBlock), uu[k], vv[k]);
    // (clamped to the frame's last ROI pixel: the tail of a camera's last tile loads in bounds and stores nothing)
    const uint32_t off = vv[k] * g.row_stride + uu[k] * elem_bytes<DT>();
    d[k] = load_disparity<DT>(fin, off < g.last_off ? off : g.last_off, g.scale);
  }
}

template <bool NT>
__device__ __forceinline__ void rig_store(v4f *out, uint32_t *out_index, uint32_t pos, float X, float Y, float Z, uint32_t pix) {
  const v4f p = {X, Y, Z, 1.0f};
  st<NT>(out + uint64_t(pos), p);
  if (out_index) out_index[uint64_t(pos)] = pix;
}

template <int DT>
__global__ __launch_bounds__(kBlock) void k_rig_parity(const uint8_t *__restrict__ frames, v4f *__restrict__ out,
                                                       uint32_t *__restrict__ out_index, uint32_t *__restrict__ counts,
                                                       uint32_t *__restrict__ offsets, const RigCal *__restrict__ table,
                                                       const Geom g, const uint32_t cv4, const uint32_t frame_pixels) {
  constexpr int S = kRigParityPxt;
  const uint32_t f = blockIdx.y, lt = blockIdx.x;
  const uint32_t base = lt * uint32_t(kBlock * S) + threadIdx.x;
  const uint32_t first = f * g.roi_n;
  float d[S];
  uint32_t uu[S], vv[S];
  rig_load<DT, S>(d, uu, vv, frames + uint64_t(f) * g.in_frame_stride, g, base);
  with_camera_q(table[f], cv4, [&](const auto &Q) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      const uint32_t i = base + uint32_t(k) * uint32_t(kBlock);
      float X, Y, Z;
      reproject(Q, uu[k], vv[k], d[k], X, Y, Z);
      if (i < g.roi_n)
        rig_store<D2PC_STORE_NT != 0>(out, out_index, first + i, X, Y, Z, f * frame_pixels + vv[k] * g.width + uu[k]);
    }
  });
  if (lt == 0 && threadIdx.x == 0) {
    if (counts) counts[f] = g.roi_n;
    if (offsets) {
      offsets[f] = first;
      if (f + 1u == g.n_frames) offsets[f + 1u] = first + g.roi_n;
    }
  }
}

// Count: every wave leaves the survivors of its own pixels (4 words per tile); no LDS, no barrier.
template <int DT>
__global__ __launch_bounds__(kBlock) void k_rig_count(const uint8_t *__restrict__ frames, uint32_t *__restrict__ tiles,
                                                      const RigCal *__restrict__ table, const Geom g, const uint32_t cv4) {
  constexpr int S = kRigCompactPxt;
  const uint32_t f = blockIdx.y, lt = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t base = lt * uint32_t(kBlock * S) + threadIdx.x;
  float d[S];
  uint32_t uu[S], vv[S];
  rig_load<DT, S>(d, uu, vv, frames + uint64_t(f) * g.in_frame_stride, g, base);
  uint32_t c = 0;
  with_camera_q(table[f], cv4, [&](const auto &Q) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      float X, Y, Z;
      reproject(Q, uu[k], vv[k], d[k], X, Y, Z);
      const bool ok = base + uint32_t(k) * uint32_t(kBlock) < g.roi_n && point_is_valid(X, Y, Z, d[k], g.min_disparity);
      c += uint32_t(__popcll(__ballot(ok)));
    }
  });
  if (lane == 0) tiles[(uint64_t(f) * g.tiles_per_frame + lt) * 4u + wave] = c;
}

// Scan: ONE block over all tiles of all cameras, kRigScanTrip tiles per trip (4 consecutive tiles per thread; the next
// trip's counts are requested before this trip's block scan).  Leaves tile i's first position in tiles[4 i], camera
// f's in offsets[f], the total in offsets[n], and counts[f] = offsets[f + 1] - offsets[f].
__global__ __launch_bounds__(kRigScanThreads) void k_rig_scan(uint32_t *tiles, uint32_t *__restrict__ counts,
                                                              uint32_t *__restrict__ offsets, const Geom g) {
  constexpr int P = int(kRigScanPerThread);
  __shared__ uint32_t s_w[kRigScanThreads / 64];
  __shared__ uint32_t s_off[kRigMaxCameras + 1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t T = g.total_tiles;
  const uint4 *part = reinterpret_cast<const uint4 *>(tiles);
  uint4 p[P];
  auto fetch = [&](uint32_t t0) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const uint32_t i = t0 + tid * uint32_t(P) + uint32_t(k);
      p[k] = i < T ? part[i] : uint4{0u, 0u, 0u, 0u};
    }
  };
  fetch(0);
  uint32_t carry = 0;
  for (uint32_t t0 = 0; t0 < T; t0 += kRigScanTrip) {
    uint32_t tot[P], mine = 0;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      tot[k] = p[k].x + p[k].y + p[k].z + p[k].w;
      mine += tot[k];
    }
    if (T - t0 > kRigScanTrip) fetch(t0 + kRigScanTrip);  // (block-uniform)
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t n = __shfl_up(incl, o, 64);
      if (lane >= uint32_t(o)) incl += n;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kRigScanThreads / 64; ++w) {
      const uint32_t x = s_w[w];
      before += w < wave ? x : 0u;
      total += x;
    }
    uint32_t run = carry + before + incl - mine;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const uint32_t i = t0 + tid * uint32_t(P) + uint32_t(k);
      if (i < T) {
        tiles[4u * uint64_t(i)] = run;
        const uint32_t f = fdiv(i, g.div_tpf);
        if (i == f * g.tiles_per_frame) s_off[f] = run;
      }
      run += tot[k];
    }
    carry += total;
    __syncthreads();  // s_w is written again by the next trip
  }
  if (tid == 0) s_off[g.n_frames] = carry;
  __syncthreads();
  if (tid <= g.n_frames) offsets[tid] = s_off[tid];
  if (tid < g.n_frames) counts[tid] = s_off[tid + 1u] - s_off[tid];
}

// Scatter: the tile's points again, placed by ballot + mbcnt behind the tile's start and the counts of the (slot, wave)
// cells before this one in the tile (LDS).
template <int DT>
__global__ __launch_bounds__(kBlock) void k_rig_scatter(const uint8_t *__restrict__ frames, v4f *__restrict__ out,
                                                        uint32_t *__restrict__ out_index, const uint32_t *__restrict__ tiles,
                                                        const RigCal *__restrict__ table, const Geom g, const uint32_t cv4,
                                                        const uint32_t frame_pixels, const uint32_t capacity) {
  constexpr int S = kRigCompactPxt, CELLS = S * (kBlock / 64);
  __shared__ uint32_t s_cnt[CELLS];
  const uint32_t f = blockIdx.y, lt = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t base = lt * uint32_t(kBlock * S) + threadIdx.x;
  const uint32_t start = tiles[(uint64_t(f) * g.tiles_per_frame + lt) * 4u];  // (uniform) left by k_rig_scan
  float d[S], X[S], Y[S], Z[S];
  uint32_t uu[S], vv[S];
  uint64_t mask[S];
  rig_load<DT, S>(d, uu, vv, frames + uint64_t(f) * g.in_frame_stride, g, base);
  with_camera_q(table[f], cv4, [&](const auto &Q) {
#pragma unroll
    for (int k = 0; k < S; ++k) {
      reproject(Q, uu[k], vv[k], d[k], X[k], Y[k], Z[k]);
      const bool ok = base + uint32_t(k) * uint32_t(kBlock) < g.roi_n && point_is_valid(X[k], Y[k], Z[k], d[k], g.min_disparity);
      mask[k] = __ballot(ok);
    }
  });
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < S; ++k) s_cnt[k * (kBlock / 64) + int(wave)] = uint32_t(__popcll(mask[k]));
  }
  __syncthreads();
  uint32_t run = start, first[S];
#pragma unroll
  for (int c = 0; c < CELLS; ++c) {  // pixel order inside the tile = (slot, wave) row-major
    if (uint32_t(c % (kBlock / 64)) == wave) first[c / (kBlock / 64)] = run;
    run += s_cnt[c];
  }
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const uint32_t pos = first[k] + mbcnt64(mask[k]);
    // pos < capacity always holds for the scan's starts; the guard keeps a stale table of starts from storing out of bounds
    if (((mask[k] >> lane) & 1ull) != 0 && pos < capacity)
      rig_store<D2PC_SCATTER_STORE_NT != 0>(out, out_index, pos, X[k], Y[k], Z[k], f * frame_pixels + vv[k] * g.width + uu[k]);
  }
}

// ---- k_texture: a producer's points + a per-pixel plane -> 32-byte PointXYZI / PointXYZRGB records -------------------
// A gather and nothing else (no reprojection arithmetic): per point 16 B read, 4 B of index (none in the PARITY
// layout), 1-4 B of texture, 32 B written.  Positions are 32-bit, every address is formed in 64 bits.
// Store mapping: one lane per 16-byte HALF record -- the even lane of a pair copies the point, the odd lane reads index
// and texture and stores {word, 0, 0, 0} -- so every store instruction of a wave writes 1 KiB contiguously.  The
// alternative, one lane per record with two 16-byte stores 32 bytes apart, is built by -DD2PC_TEXTURE_LANE_PER_RECORD=1
// (`make variant`) for tools/ab_texture.sh only: it is 4-13 % slower at every size but one tie (profiles/texture_ab.txt).
#ifndef D2PC_TEXTURE_LANE_PER_RECORD
#define D2PC_TEXTURE_LANE_PER_RECORD 0
#endif
constexpr uint64_t kTexMaxBlocks = 1u << 16;
constexpr int kTexSlots = 4;  // records (half records) in flight per lane

// Where the sample of source pixel `pix` of cloud c lies; a pixel outside the declared planes (ok = false) gets the
// address of pixel 0 of a declared plane, so that the load stays unconditional and inside the planes: its value is dropped.
__device__ __forceinline__ const uint8_t *texture_addr(const TexArgs &a, uint32_t c, uint32_t pix, uint32_t bpp, bool &ok) {
  ok = uint64_t(pix) < a.pixel_limit;
  pix = ok ? pix : 0u;
  uint32_t f = c;
  if (a.merged) {  // (launch-uniform)
    f = fdiv(pix, a.div_frame);
    pix -= f * a.frame_pixels;
  }
  const uint32_t v = fdiv(pix, a.div_w), u = pix - v * a.width;
  return a.tex + uint64_t(f) * a.tex_frame_stride + uint64_t(v) * uint64_t(a.tex_pitch) + uint64_t(u * bpp);
}

// The texture words of a lane's kTexSlots records: ONE launch-uniform switch around the loads of all slots, so that they
// are in flight together.  The source pixel of record i is the producer's index, or the PARITY layout's ROI pixel.
__device__ __forceinline__ void texture_words(const TexArgs &a, const uint32_t *index, uint32_t c,
                                              const uint32_t (&rec)[kTexSlots], uint32_t (&w)[kTexSlots]) {
  uint32_t pix[kTexSlots];
  if (index) {
#pragma unroll
    for (int k = 0; k < kTexSlots; ++k) pix[k] = index[uint64_t(rec[k])];
  } else {
#pragma unroll
    for (int k = 0; k < kTexSlots; ++k) {
      const uint32_t rv = fdiv(rec[k], a.div_roi_w);
      pix[k] = (rv + a.border) * a.width + (rec[k] - rv * a.roi_w) + a.border;
    }
  }
  const uint32_t kind = a.kind;
  const uint32_t bpp = kind == TEX_U16 ? 2u : kind == TEX_F32 ? 4u : (kind == TEX_RGB8 || kind == TEX_BGR8) ? 3u : 1u;
  const uint8_t *q[kTexSlots];
  bool ok[kTexSlots];
#pragma unroll
  for (int k = 0; k < kTexSlots; ++k) q[k] = texture_addr(a, c, pix[k], bpp, ok[k]);
  switch (kind) {
    case TEX_U8:
#pragma unroll
      for (int k = 0; k < kTexSlots; ++k) w[k] = __float_as_uint(float(q[k][0]));
      break;
    case TEX_U16:
#pragma unroll
      for (int k = 0; k < kTexSlots; ++k) w[k] = __float_as_uint(float(*reinterpret_cast<const uint16_t *>(q[k])));
      break;
    case TEX_F32:
#pragma unroll
      for (int k = 0; k < kTexSlots; ++k) w[k] = *reinterpret_cast<const uint32_t *>(q[k]);
      break;
    case TEX_MONO8:
#pragma unroll
      for (int k = 0; k < kTexSlots; ++k) w[k] = 0xff000000u | uint32_t(q[k][0]) * 0x010101u;
      break;
    default: {
      uint32_t p0[kTexSlots], p1[kTexSlots], p2[kTexSlots];
#pragma unroll
      for (int k = 0; k < kTexSlots; ++k) p0[k] = q[k][0], p1[k] = q[k][1], p2[k] = q[k][2];
#pragma unroll
      for (int k = 0; k < kTexSlots; ++k)
        w[k] = 0xff000000u | p1[k] << 8 | (kind == TEX_RGB8 ? p0[k] << 16 | p2[k] : p2[k] << 16 | p0[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kTexSlots; ++k) w[k] = ok[k] ? w[k] : 0u;
}

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// Loads are unconditional -- a position past the count is clamped to the cloud's last record (the loop runs only for
// n >= 1), whose bytes are read and dropped -- so that the loads of all slots are issued before the first wait; only
// the stores are predicated.
template <bool HALF>
__global__ __launch_bounds__(kBlock) void k_texture(const TexArgs a) {
  static_assert(kTexSlots == 4, "the point slots are named");
  const uint32_t c = blockIdx.y;
  uint32_t n = a.cloud_points;
  if (a.counts) {
    const uint32_t k = a.counts[c];
    n = k == kCountTimedOut ? 0u : (k < n ? k : n);
  }
  const v4u *pts = static_cast<const v4u *>(a.points) + uint64_t(c) * a.points_stride;
  const uint32_t *index = a.index ? a.index + uint64_t(c) * a.points_stride : nullptr;
  v4u *out = static_cast<v4u *>(a.out) + 2u * uint64_t(c) * a.out_stride;  // in 16-byte halves
  constexpr uint32_t kStep = HALF ? uint32_t(kBlock) / 2u : uint32_t(kBlock), kTile = kStep * uint32_t(kTexSlots);
  const uint32_t lane_rec = HALF ? threadIdx.x >> 1 : threadIdx.x, odd = threadIdx.x & 1u;
  const uint32_t last = n - 1u;
  for (uint64_t r0 = uint64_t(blockIdx.x) * kTile; r0 < n; r0 += uint64_t(gridDim.x) * kTile) {
    const uint64_t i0 = r0 + lane_rec, i1 = i0 + kStep, i2 = i1 + kStep, i3 = i2 + kStep;
    const uint32_t rec[kTexSlots] = {i0 < n ? uint32_t(i0) : last, i1 < n ? uint32_t(i1) : last,
                                     i2 < n ? uint32_t(i2) : last, i3 < n ? uint32_t(i3) : last};
    uint32_t w[kTexSlots];
    if constexpr (!HALF) {
      const v4u p0 = pts[uint64_t(rec[0])], p1 = pts[uint64_t(rec[1])], p2 = pts[uint64_t(rec[2])], p3 = pts[uint64_t(rec[3])];
      texture_words(a, index, c, rec, w);
      if (i0 < n) out[2u * i0] = p0, out[2u * i0 + 1u] = v4u{w[0], 0u, 0u, 0u};
      if (i1 < n) out[2u * i1] = p1, out[2u * i1 + 1u] = v4u{w[1], 0u, 0u, 0u};
      if (i2 < n) out[2u * i2] = p2, out[2u * i2 + 1u] = v4u{w[2], 0u, 0u, 0u};
      if (i3 < n) out[2u * i3] = p3, out[2u * i3 + 1u] = v4u{w[3], 0u, 0u, 0u};
    } else {
      v4u h0, h1, h2, h3;
      if (odd) {  // one divergence for the four slots: the odd lanes' index and sample loads, the even lanes' point loads
        texture_words(a, index, c, rec, w);
        h0 = v4u{w[0], 0u, 0u, 0u}, h1 = v4u{w[1], 0u, 0u, 0u}, h2 = v4u{w[2], 0u, 0u, 0u}, h3 = v4u{w[3], 0u, 0u, 0u};
      } else {
        h0 = pts[uint64_t(rec[0])], h1 = pts[uint64_t(rec[1])], h2 = pts[uint64_t(rec[2])], h3 = pts[uint64_t(rec[3])];
      }
      if (i0 < n) out[2u * i0 + odd] = h0;
      if (i1 < n) out[2u * i1 + odd] = h1;
      if (i2 < n) out[2u * i2 + odd] = h2;
      if (i3 < n) out[2u * i3 + odd] = h3;
    }
  }
}

hipError_t launch_texture(const TexArgs &a) {
  constexpr bool half = D2PC_TEXTURE_LANE_PER_RECORD == 0;
  const uint64_t tile = uint64_t(kBlock) / (half ? 2u : 1u) * kTexSlots;
  // one-shot blocks up to 2^16 per cloud (33 million records), a stride loop beyond; a block past the cloud's count
  // leaves at once
  const uint64_t tiles = (uint64_t(a.cloud_points) + tile - 1) / tile;
  const dim3 grid(uint32_t(tiles < kTexMaxBlocks ? tiles : kTexMaxBlocks), a.n_clouds);
  hipLaunchKernelGGL(k_texture<half>, grid, dim3(kBlock), 0, a.stream, a);
  return hipGetLastError();
}

hipError_t launch_rig_parity(const RigArgs &a) {
  return for_dtype(a.dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL((k_rig_parity<DT>), dim3(a.geom.tiles_per_frame, a.geom.n_frames), dim3(kBlock), 0, a.stream,
                       static_cast<const uint8_t *>(a.frames), static_cast<v4f *>(a.out_points), a.out_index, a.counts, a.offsets,
                       a.table, a.geom, a.cv4, a.frame_pixels);
    return hipGetLastError();
  });
}

hipError_t launch_rig_compact(const RigArgs &a) {
  return for_dtype(a.dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const dim3 grid(a.geom.tiles_per_frame, a.geom.n_frames);
    const uint8_t *frames = static_cast<const uint8_t *>(a.frames);
    hipLaunchKernelGGL((k_rig_count<DT>), grid, dim3(kBlock), 0, a.stream, frames, a.tiles, a.table, a.geom, a.cv4);
    hipLaunchKernelGGL(k_rig_scan, dim3(1), dim3(kRigScanThreads), 0, a.stream, a.tiles, a.counts, a.offsets, a.geom);
    const uint64_t cap = uint64_t(a.geom.roi_n) * a.geom.n_frames;
    hipLaunchKernelGGL((k_rig_scatter<DT>), grid, dim3(kBlock), 0, a.stream, frames, static_cast<v4f *>(a.out_points), a.out_index,
                       a.tiles, a.table, a.geom, a.cv4, a.frame_pixels, uint32_t(cap));
    return hipGetLastError();
  });
}

}  // namespace d2pc
