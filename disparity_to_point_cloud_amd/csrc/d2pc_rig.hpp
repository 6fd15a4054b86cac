// d2pc_rig.hpp -- launch interface between the rig session of the C ABI (d2pc_capi_rig.hip) and its kernels
// (d2pc_rig.hip): N cameras of one geometry, one Q each, one merged cloud.
#pragma once

#include "d2pc_launch.hpp"

namespace d2pc {

// One camera's calibration as the kernels read it from DEVICE memory (a block serves one camera: the entry is
// wave-uniform and arrives through scalar loads).  Filled by the host when a Q is set.
struct RigCal {
  double q[16];            // Q, row-major, bit copy
  double cx, cy, f, a, b;  // the stereo constants as classify_q forms them (d2pc_capi_context.hip)
  double f_cv4;            // double(float(f)): Z's numerator under D2PC_FORM_CV4 (fill_q)
  uint32_t stereo;         // 1: Q has cv::stereoRectify's structure
  uint32_t pad;
};
static_assert(sizeof(RigCal) == 184, "the table's entries are 184 bytes");

constexpr int kRigMaxCameras = 64;         // = D2PC_RIG_MAX_CAMERAS
constexpr int kRigParityPxt = 2;             // PARITY: one-shot blocks of 512 ROI pixels
constexpr int kRigCompactPxt = 4;            // COMPACT: tiles of 1,024 ROI pixels in count and scatter
constexpr uint32_t kRigScanThreads = 1024;   // the one scan block ...
constexpr uint32_t kRigScanPerThread = 4;    // ... takes 4 consecutive tiles per thread and trip
constexpr uint32_t kRigScanTrip = kRigScanThreads * kRigScanPerThread;

struct RigArgs {
  const void *frames = nullptr;   // device: geom.n_frames frames, geom.in_frame_stride apart
  void *out_points = nullptr;     // device: the merged cloud
  uint32_t *out_index = nullptr;  // device, nullable
  uint32_t *counts = nullptr;     // device: n (nullable in PARITY)
  uint32_t *offsets = nullptr;    // device: n + 1 (nullable in PARITY)
  const RigCal *table = nullptr;  // device: n entries
  uint32_t *tiles = nullptr;      // device: 4 words per COMPACT tile (wave counts, then the tile's start in word 0)
  int dtype = DT_F32;
  uint32_t cv4 = 0;               // 1: D2PC_FORM_CV4, 0: D2PC_FORM_DEFAULT
  uint32_t frame_pixels = 0;      // W * H mod 2^32 (the index of camera f starts at f * W * H)
  Geom geom{};                    // PARITY: in tiles of 256 * kRigParityPxt, COMPACT: of 256 * kRigCompactPxt
  hipStream_t stream = nullptr;
};

hipError_t launch_rig_parity(const RigArgs &a);
hipError_t launch_rig_compact(const RigArgs &a);  // count, scan, scatter

// d2pc_texture_device: the gather that turns a producer's 16-byte points into 32-byte PointXYZI / PointXYZRGB records
// (k_texture lives beside the rig's kernels to share their code object: a translation unit of its own costs ~10 KB of
// the product library's size budget).
enum : uint32_t { TEX_U8 = 0, TEX_U16 = 1, TEX_F32 = 2, TEX_RGB8 = 3, TEX_BGR8 = 4, TEX_MONO8 = 5 };
struct TexArgs {
  const uint8_t *tex = nullptr;     // device: n_frames planes
  const void *points = nullptr;     // device: 16-byte records
  const uint32_t *index = nullptr;  // device, nullable (PARITY layout)
  const uint32_t *counts = nullptr; // device, nullable
  void *out = nullptr;              // device: 32-byte records
  uint64_t tex_frame_stride = 0;    // bytes
  uint64_t points_stride = 0;       // points between clouds (points and index)
  uint64_t out_stride = 0;          // records between clouds
  uint64_t pixel_limit = 0;         // an index at or beyond it reads nothing: W * H, merged: n_frames * W * H (<= 2^32)
  uint32_t tex_pitch = 0;           // bytes (< 2^32; row * pitch is formed in 64 bits)
  uint32_t cloud_points = 0;
  uint32_t n_clouds = 0;            // grid.y
  uint32_t width = 0, frame_pixels = 0;
  uint32_t border = 0, roi_w = 0;   // PARITY layout only
  uint32_t kind = TEX_U8;
  uint32_t merged = 0;
  FastDiv div_w{}, div_frame{}, div_roi_w{};
  hipStream_t stream = nullptr;
};
hipError_t launch_texture(const TexArgs &a);

}  // namespace d2pc
