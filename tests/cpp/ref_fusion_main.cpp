// ref_fusion_main.cpp -- the compiled reference (oracle/ref_shim/ref_harness.cpp + the reference's own
// depth_map_fusion.cpp + the stand-in headers) as a stand-alone program for -fsanitize=address,undefined:
// tests/test_reference_cpu.py builds and runs it.  The three OpenCV filters are identity copies here: the program is
// about memory and undefined behaviour in the stand-ins, the harness and the reference's indexing, not about values.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ref_harness.h"

namespace {

int copy_view(const ref_view *src, const ref_view *dst) {
  if (src->rows != dst->rows || src->cols != dst->cols) return 1;
  for (int i = 0; i < src->rows; ++i)
    std::memmove(dst->data + size_t(i) * dst->step, src->data + size_t(i) * src->step, size_t(src->cols));
  return 0;
}
int gaussian(const ref_view *src, const ref_view *dst, int, int, double) {
  // read the corners of the allocation the view lies in, as a border-reading filter would
  const unsigned char *p = src->parent;
  volatile unsigned char sink = p[0];
  sink = p[size_t(src->parent_rows - 1) * src->step + size_t(src->parent_cols - 1)];
  (void)sink;
  return copy_view(src, dst);
}
int sobel(const ref_view *src, const ref_view *dst, int, int, int, double) { return copy_view(src, dst); }
int threshold(const ref_view *src, const ref_view *dst, double, double, int) { return copy_view(src, dst); }

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      return 1;                                                        \
    }                                                                  \
  } while (0)

int run_script(int cols, int rows, int offset_x, int offset_y, const std::vector<int> &calls, int want_topics) {
  ref_node *node = ref_node_create(offset_x, offset_y, 1, 1);
  std::vector<uint8_t> frame(size_t(cols + 3) * size_t(rows));
  uint32_t x = 12345u + uint32_t(cols);
  int topics = 0;
  for (size_t k = 0; k < calls.size(); ++k) {
    for (uint8_t &b : frame) b = uint8_t((x = x * 1664525u + 1013904223u) >> 24);
    CHECK(ref_node_callback(node, calls[k], frame.data(), size_t(cols + 3), cols, rows, uint32_t(k), "cam") == REF_OK);
    for (int i = 0; i < ref_node_published(node); ++i) {
      ref_topic t;
      CHECK(ref_node_topic(node, i, &t) == REF_OK);
      CHECK(t.bytes == size_t(t.step) * t.height && t.step == t.width * (std::strcmp(t.encoding, "rgb8") ? 1u : 3u));
      unsigned sum = 0;
      for (size_t b = 0; b < t.bytes; ++b) sum += t.data[b];  // every published byte is readable
      (void)sum;
      ++topics;
    }
  }
  ref_node_destroy(node);
  CHECK(topics == want_topics);
  return 0;
}

}  // namespace

int main() {
  // a filter without a hook is a status, not a crash
  {
    ref_node *node = ref_node_create(0, 0, 1, 1);
    std::vector<uint8_t> f(75 * 58, 9);
    CHECK(ref_node_callback(node, REF_MATCHING_SCORE_1, f.data(), 75, 75, 58, 0, "cam") == REF_NO_HOOK);
    ref_node_destroy(node);
  }
  ref_set_hooks(gaussian, sobel, threshold);
  const int D1 = REF_DISPARITY_1, D2 = REF_DISPARITY_2, S1 = REF_MATCHING_SCORE_1, S2 = REF_MATCHING_SCORE_2;
  // landscape: D2 before anything else, then all planes, D2 twice, S1 between two D2
  if (run_script(75, 58, -2, 5, {D2, S1, D1, S2, D2, D2, S1, D2, S2, D1}, 1 + 1 + 1 + 1 + 4 + 4 + 1 + 4 + 1 + 1)) return 1;
  // portrait, the other signs, |offset_x| = |offset_y|
  if (run_script(58, 75, 4, -4, {S2, S1, D1, D2, D2, S2, D2}, 1 + 1 + 1 + 4 + 4 + 1 + 4)) return 1;

  // the pure queries: a throwing crop is an outcome
  int rect[16];
  CHECK(ref_crop_to_square(752, 480, -7, 15, 15, rect) == REF_OK && rect[0] == 133 && rect[1] == 15 && rect[2] == 465);
  CHECK(ref_crop_to_square(11, 11, 0, 0, 20, rect) == REF_THREW);
  CHECK(ref_crop_mat(39, 39, 0, 40, 30, 10, rect) == REF_THREW);
  CHECK(ref_geometry(200, 140, 9, -6, rect) == 0 && rect[2] == 131 && rect[10] == 134 && rect[14] == 94);
  CHECK(ref_geometry(11, 41, 20, -20, rect) != 0);
  std::vector<uint8_t> gray(256), rgb(768), a(65536), b(65536), s(65536, 99), rot(15);
  for (int i = 0; i < 256; ++i) gray[size_t(i)] = uint8_t(i);
  CHECK(ref_colorize(gray.data(), 16, 16, 16, 1, rgb.data()) == REF_OK && rgb[0] == 0 && rgb[5] == 0 && rgb[6] + rgb[7] + rgb[8] > 0);
  int size[2];
  CHECK(ref_rotate_mat(gray.data(), 5, 5, 3, rot.data(), size) == REF_OK && size[0] == 3 && size[1] == 5 && rot[0] == 10 && rot[2] == 0);
  for (int i = 0; i < 65536; ++i) a[size_t(i)] = uint8_t(i >> 8), b[size_t(i)] = uint8_t(i);
  std::vector<int16_t> out(65536);
  for (int rule = 0; rule < 9; ++rule) CHECK(ref_fuse_pixels(rule, out.size(), a.data(), b.data(), s.data(), s.data(), nullptr, nullptr, out.data()) == REF_OK);
  CHECK(out[size_t(100 * 256 + 100)] == 100);  // gradFilter: equal depths, equal scores below 125: their mean
  std::printf("ref_fusion_main ok\n");
  return 0;
}
