// d2pc_plane.hpp -- one image plane as a caller hands it to the C ABI (pointer, pitch, frame stride, rows x row bytes
// x frames) and the three questions every image entry point asks of it: does it fit, which bytes does it span, which
// frame stride does the kernel get.  Host code only and no HIP: plain g++ compiles it (tests/cpp/plane_check_main.cpp
// checks it against a byte-by-byte model).  Sizes are size_t and are not checked for wrap-around.
#pragma once
#include <cstddef>
#include <cstdint>

namespace d2pc {
namespace host {

// What has to fit 32 bits.  Plane: pitch * rows, for kernels that form a row's offset (row * pitch) in 32 bits.
// Pitch: the pitch alone, for kernels that form it in 64 bits from a 32-bit pitch.
enum class Bound32 { Plane, Pitch };
// The smallest frame stride of a batch.  LastRow: a frame ends with the last byte of its last row.  WholeRows:
// it ends with the whole pitch of its last row (the median entry points).
enum class FrameRule { LastRow, WholeRows };

struct Plane {
  const void *p;
  size_t pitch, frame_stride;  // bytes; the frame stride counts for n_frames > 1 only
  size_t row_bytes;
  int rows;

  bool empty() const { return rows <= 0 || row_bytes == 0; }
  size_t frame_extent() const { return size_t(rows - 1) * pitch + row_bytes; }
  // bytes from p to one past the last byte a kernel may touch (0: an empty plane touches none)
  size_t extent(int n_frames) const { return empty() ? 0 : size_t(n_frames - 1) * frame_stride + frame_extent(); }
  bool fits(int n_frames, Bound32 bound, FrameRule rule = FrameRule::LastRow) const {
    if (pitch < row_bytes) return false;
    if ((bound == Bound32::Plane ? pitch * size_t(rows) : pitch) > 0xffffffffull) return false;
    return n_frames <= 1 || frame_stride >= (rule == FrameRule::WholeRows ? size_t(rows) * pitch : frame_extent());
  }
  // what the launch structs carry: a single frame has no stride
  size_t kernel_frame_stride(int n_frames) const { return n_frames > 1 ? frame_stride : 0; }
};

// Do the hulls [p, p + extent) intersect?  Interleaved slices whose hulls intersect count as overlapping although
// they share no byte: the refusal is conservative on purpose.  A null plane overlaps nothing.
inline bool overlaps(const Plane &a, const Plane &b, int n_frames) {
  if (!a.p || !b.p) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
  return a0 < b0 + b.extent(n_frames) && b0 < a0 + a.extent(n_frames);
}

}  // namespace host
}  // namespace d2pc
