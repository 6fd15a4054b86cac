// csrc/d2pc_plane.hpp against a model that shares none of its arithmetic: every small plane is laid into a 256-byte
// arena and the bytes it touches are marked one by one (frames x rows x columns); extent, hull and aliasing are read
// off the marks.  No HIP, no GPU: g++ -fsanitize=address,undefined (tests/test_plane_check_cpu.py).
#include <bitset>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../disparity_to_point_cloud_amd/csrc/d2pc_plane.hpp"

using d2pc::host::Bound32;
using d2pc::host::FrameRule;
using d2pc::host::Plane;
using d2pc::host::overlaps;

static_assert(sizeof(size_t) == 8, "the 2^32 edge cases need a 64-bit size_t");

namespace {

constexpr int kArena = 256, kBases = 41;
unsigned char arena[kArena];
using Bytes = std::bitset<kArena>;

struct Shape {
  size_t row_bytes, pitch, frame_stride;
  int rows, frames;
};

[[noreturn]] void die(const char *what, const Shape &s, int base) {
  std::printf("FAILED %s: row bytes %zu, rows %d, pitch %zu, frames %d, frame stride %zu, base %d\n", what, s.row_bytes,
              s.rows, s.pitch, s.frames, s.frame_stride, base);
  std::exit(1);
}

Plane plane_of(const Shape &s, int base) { return Plane{arena + base, s.pitch, s.frame_stride, s.row_bytes, s.rows}; }

// the model: mark every byte of every row of every frame
Bytes touched(const Shape &s, int base) {
  Bytes b;
  for (int f = 0; f < s.frames; ++f)
    for (int r = 0; r < s.rows; ++r)
      for (size_t c = 0; c < s.row_bytes; ++c) b.set(size_t(base) + size_t(f) * s.frame_stride + size_t(r) * s.pitch + c);
  return b;
}

int first(const Bytes &b) {
  for (int i = 0; i < kArena; ++i)
    if (b[size_t(i)]) return i;
  return -1;
}

int last(const Bytes &b) {
  for (int i = kArena - 1; i >= 0; --i)
    if (b[size_t(i)]) return i;
  return -1;
}

// the three inequalities of the fit test, written out
bool model_fits(const Shape &s, bool bound_plane, bool whole_rows) {
  if (!(s.pitch >= s.row_bytes)) return false;
  if (bound_plane && !(s.pitch * size_t(s.rows) <= 0xffffffffull)) return false;
  if (!bound_plane && !(s.pitch <= 0xffffffffull)) return false;
  if (s.frames > 1 && whole_rows && !(s.frame_stride >= size_t(s.rows) * s.pitch)) return false;
  if (s.frames > 1 && !whole_rows && !(s.frame_stride >= size_t(s.rows - 1) * s.pitch + s.row_bytes)) return false;
  return true;
}

void check_fits(const Shape &s, int base, const char *what) {
  const Plane p = plane_of(s, base);
  for (int bp = 0; bp < 2; ++bp)
    for (int wr = 0; wr < 2; ++wr)
      if (p.fits(s.frames, bp ? Bound32::Plane : Bound32::Pitch, wr ? FrameRule::WholeRows : FrameRule::LastRow) !=
          model_fits(s, bp, wr))
        die(what, s, base);
}

}  // namespace

int main() {
  std::vector<Shape> shapes[4];  // by frame count
  for (int frames = 1; frames <= 3; ++frames)
    for (size_t rb = 1; rb <= 4; ++rb)
      for (int rows = 1; rows <= 3; ++rows)
        for (size_t pitch = 0; pitch <= 6; ++pitch)
          for (size_t fs = 0; fs <= 20; ++fs) shapes[frames].push_back(Shape{rb, pitch, fs, rows, frames});

  size_t n_planes = 0, n_pairs = 0, n_alias = 0, n_hull_only = 0;
  for (int frames = 1; frames <= 3; ++frames) {
    const std::vector<Shape> &all = shapes[frames];
    for (size_t i = 0; i < all.size(); ++i) {
      const Shape &s = all[i];
      for (int base = 0; base < kBases; ++base, ++n_planes) {
        const Plane p = plane_of(s, base);
        const Bytes mine = touched(s, base);
        if (first(mine) != base) die("first byte", s, base);
        if (p.extent(frames) != size_t(last(mine) - base + 1)) die("extent", s, base);
        check_fits(s, base, "fits");
        if (p.kernel_frame_stride(frames) != (frames == 1 ? 0 : s.frame_stride)) die("kernel_frame_stride", s, base);
        if ((p.kernel_frame_stride(frames) == 0) != (frames == 1 || s.frame_stride == 0)) die("kernel_frame_stride zero", s, base);
        // partners of the same frame count: the same shape, and two that walk through all shapes as plane and base vary
        const size_t partner[3] = {i, (i * 7 + size_t(base) * 131 + 1) % all.size(), (i * 5003 + size_t(base) * 17 + 3) % all.size()};
        const int partner_base[3] = {20, 20, (base * 3 + 11) % kBases};
        for (int k = 0; k < 3; ++k, ++n_pairs) {
          const Shape &t = all[partner[k]];
          const Plane q = plane_of(t, partner_base[k]);
          const Bytes theirs = touched(t, partner_base[k]);
          const int lo = first(mine) > first(theirs) ? first(mine) : first(theirs);
          const int hi = last(mine) < last(theirs) ? last(mine) : last(theirs);
          const bool hulls = lo <= hi, alias = (mine & theirs).any();
          if (overlaps(p, q, frames) != hulls || overlaps(q, p, frames) != hulls) die("overlaps != hull intersection", s, base);
          if (alias && !overlaps(p, q, frames)) die("a true alias was missed", s, base);
          n_alias += alias, n_hull_only += hulls && !alias;
        }
      }
    }
  }
  if (n_alias == 0 || n_hull_only == 0 || n_alias + n_hull_only == n_pairs) {
    std::printf("FAILED: the pairs do not cover aliasing, interleaved and disjoint planes\n");
    return 1;
  }

  // a null plane overlaps nothing; an empty plane touches nothing
  const Shape some{4, 6, 20, 3, 3};
  const Plane whole{arena, 6, 20, 4, 3}, null{nullptr, 6, 20, 4, 3};
  if (overlaps(null, whole, 3) || overlaps(whole, null, 3) || overlaps(null, null, 3)) die("null plane", some, 0);
  if (Plane{arena, 6, 20, 0, 3}.extent(3) != 0 || Plane{arena, 6, 20, 4, 0}.extent(3) != 0 || !Plane{arena, 6, 20, 4, 0}.empty() ||
      whole.empty())
    die("empty plane", some, 0);

  // the 2^32 edges: where the two bounds agree and where they differ
  struct Edge { size_t pitch; int rows; bool plane_ok, pitch_ok; };
  const Edge edges[] = {
      {0x55555555ull, 3, true, true},     // pitch * rows == 0xffffffff
      {0x40000000ull, 4, false, true},    // pitch * rows == 0x100000000
      {0xffffffffull, 1, true, true},     // pitch == 0xffffffff, one row
      {0xffffffffull, 2, false, true},    // ... two rows: only the plane bound refuses
      {0x100000000ull, 1, false, false},  // pitch == 0x100000000
  };
  for (const Edge &e : edges) {
    const Shape s{1, e.pitch, 0, e.rows, 1};
    const Plane p{nullptr, e.pitch, 0, 1, e.rows};
    if (p.fits(1, Bound32::Plane) != e.plane_ok || p.fits(1, Bound32::Pitch) != e.pitch_ok) die("2^32 edge", s, 0);
    check_fits(s, 0, "2^32 edge against the model");
    // a batch: the frame-stride rules at these sizes
    const Shape b{1, e.pitch, e.pitch * size_t(e.rows - 1) + 1, e.rows, 2};
    const Plane pb{nullptr, b.pitch, b.frame_stride, 1, b.rows};
    check_fits(b, 0, "2^32 edge, two frames");
    if (pb.fits(2, Bound32::Pitch) != e.pitch_ok) die("2^32 edge, last-row frame stride", b, 0);
    if (e.pitch > 1 && pb.fits(2, Bound32::Pitch, FrameRule::WholeRows)) die("2^32 edge, whole-rows frame stride", b, 0);
  }
  std::printf("plane check ok: %zu planes, %zu pairs (%zu aliasing, %zu with intersecting hulls only)\n", n_planes, n_pairs,
              n_alias, n_hull_only);
  return 0;
}
