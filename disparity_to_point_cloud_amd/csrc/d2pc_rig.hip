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
