// ref_harness.cpp -- a C ABI over the reference's own DepthMapFusion class, compiled together with the reference's
// unmodified depth_map_fusion.cpp against the stand-in headers of this directory (-fno-access-control opens the
// class's private members).  Nothing here computes a result: every value returned comes out of a reference function.
// Used by oracle/ref.py (through oracle/_ref/libref_fusion.so) and by tests/cpp/ref_fusion_main.cpp.
#include <cstdint>
#include <cstring>
#include <string>

#include "disparity_to_point_cloud/depth_map_fusion.hpp"
#include "ref_harness.h"

ref_filter_hooks ref_hooks = {nullptr, nullptr, nullptr};

namespace {

using depth_map_fusion::DepthMapFusion;

std::string g_error;

// a node with the given member offsets and nothing else: for calling the reference's pure member functions
DepthMapFusion *make_node(int offset_x, int offset_y) {
  ros::param_table().clear();
  ros::param_table()["offset_x"] = offset_x;
  ros::param_table()["offset_y"] = offset_y;
  return new DepthMapFusion();
}

DepthMapFusion &plain_node() {
  static DepthMapFusion *node = make_node(0, 0);
  return *node;
}

void describe(const cv::Mat &m, int out[4]) {
  cv::Size whole;
  cv::Point ofs;
  m.locateROI(whole, ofs);
  out[0] = ofs.x, out[1] = ofs.y, out[2] = m.cols, out[3] = m.rows;
}

template <class F>
int guarded(F f) {
  try {
    f();
    return REF_OK;
  } catch (const cv::HookMissing &e) {
    g_error = e.what();
    return REF_NO_HOOK;
  } catch (const std::exception &e) {
    g_error = e.what();
    return REF_THREW;
  }
}

}  // namespace

struct ref_node {
  DepthMapFusion *node;
};

extern "C" {

const char *ref_last_error(void) { return g_error.c_str(); }

void ref_set_hooks(ref_gaussian_hook gaussian, ref_sobel_hook sobel, ref_threshold_hook threshold) {
  ref_hooks.gaussian = gaussian, ref_hooks.sobel = sobel, ref_hooks.threshold = threshold;
}

int ref_fuse_pixels(int rule, size_t count, const uint8_t *d1, const uint8_t *d2, const uint8_t *s1, const uint8_t *s2,
                    const uint8_t *g1, const uint8_t *g2, int16_t *out) {
  DepthMapFusion &n = plain_node();
  typedef int (DepthMapFusion::*Rule4)(int, int, int, int);
  static const Rule4 rules[8] = {&DepthMapFusion::weightedAverage, &DepthMapFusion::maxDist, &DepthMapFusion::maxDistUnlessBlack,
                                 &DepthMapFusion::betterScore,     &DepthMapFusion::onlyGood1, &DepthMapFusion::onlyGoodAvg,
                                 &DepthMapFusion::overlap,         &DepthMapFusion::blackToWhite};
  if (rule < 0 || rule > 8) return REF_BAD_ARG;
  for (size_t i = 0; i < count; ++i) {
    if (rule == 8) {
      out[i] = int16_t(n.gradFilter(d1[i], d2[i], s1[i], s2[i], g1 ? g1[i] : 0, g2 ? g2[i] : 0));
    } else if (rule == 0 && s1[i] != 0 && s2[i] != 0) {
      out[i] = -1;  // both weights are 0: the reference would divide by zero, it is not called
    } else {
      out[i] = int16_t((n.*rules[rule])(d1[i], d2[i], s1[i], s2[i]));
    }
  }
  return REF_OK;
}

int ref_crop_to_square(int cols, int rows, int offset_x, int offset_y, int member_offset_y, int rect[4]) {
  DepthMapFusion &n = plain_node();
  const int saved = n.offset_y_;
  n.offset_y_ = member_offset_y;
  const int st = guarded([&] {
    const cv::Mat image(rows, cols, CV_8UC1);
    describe(n.cropToSquare(image, offset_x, offset_y), rect);
  });
  n.offset_y_ = saved;
  return st;
}

int ref_crop_mat(int cols, int rows, int left, int right, int top, int bottom, int rect[4]) {
  return guarded([&] {
    const cv::Mat image(rows, cols, CV_8UC1);
    describe(plain_node().cropMat(image, left, right, top, bottom), rect);
  });
}

int ref_rotate_mat(const uint8_t *src, size_t step, int cols, int rows, uint8_t *dst, int dst_size[2]) {
  return guarded([&] {
    cv::Mat image(rows, cols, CV_8UC1);
    for (int i = 0; i < rows; ++i) std::memcpy(image.data + size_t(i) * image.step, src + size_t(i) * step, size_t(cols));
    const cv::Mat rot = plain_node().rotateMat(image);
    dst_size[0] = rot.cols, dst_size[1] = rot.rows;
    for (int i = 0; i < rot.rows; ++i) std::memcpy(dst + size_t(i) * size_t(rot.cols), rot.data + size_t(i) * rot.step, size_t(rot.cols));
  });
}

int ref_colorize(const uint8_t *gray, size_t step, int cols, int rows, int as_view, uint8_t *rgb) {
  return guarded([&] {
    // as_view: the plane lies inside a larger allocation, so its rows are further apart than its width
    const int pad = as_view ? 5 : 0;
    cv::Mat whole(rows + 2 * pad, cols + 2 * pad, CV_8UC1);
    whole = cv::Scalar::all(77);
    cv::Mat plane = whole(cv::Rect(pad, pad, cols, rows));
    for (int i = 0; i < rows; ++i) std::memcpy(plane.data + size_t(i) * plane.step, gray + size_t(i) * step, size_t(cols));
    cv::Mat out;
    plain_node().colorizeDepth(plane, out);
    for (int i = 0; i < out.rows; ++i) std::memcpy(rgb + size_t(i) * size_t(cols) * 3, out.data + size_t(i) * out.step, size_t(cols) * 3);
  });
}

// The sizes of everything one full round of callbacks publishes for frames of cols x rows, by the reference's own
// cropToSquare / rotateMat / cropMat: out = sq1 (x, y, w, h), sq2 (x, y, w, h), the fuse image's square (x, y, w, h),
// the fused map (x, y, w, h) inside that square.  Returns a bit per stage that threw: 1 camera 1's square, 2 camera
// 2's, 4 the fuse image's square, 8 the crop of the fused map (also set when there was no square to crop).
int ref_geometry(int cols, int rows, int offset_x, int offset_y, int out[16]) {
  DepthMapFusion &n = plain_node();
  const int saved_x = n.offset_x_, saved_y = n.offset_y_;
  n.offset_x_ = offset_x, n.offset_y_ = offset_y;
  // the frame and its rotation (the reference's rotateMat) are kept between calls of one size: a sweep over offsets
  // would otherwise rotate the same blank frame again for every pair
  static cv::Mat frame, rot;
  if (frame.cols != cols || frame.rows != rows || rot.empty()) {
    frame = cv::Mat(rows, cols, CV_8UC1);
    rot = n.rotateMat(frame);
  }
  int threw = 0;
  if (guarded([&] { describe(n.cropToSquare(frame, n.offset_x_, n.offset_y_), out); }) != REF_OK) threw |= 1;  // DisparityCb1 / MatchingScoreCb1
  if (guarded([&] { describe(n.cropToSquare(rot, -n.offset_x_, -n.offset_y_), out + 4); }) != REF_OK) threw |= 2;  // DisparityCb2 / MatchingScoreCb2
  cv::Mat fuse;
  if (guarded([&] {
        fuse = n.cropToSquare(frame);  // publishFusedDepthMap
        describe(fuse, out + 8);
      }) != REF_OK)
    threw |= 4 | 8;
  else if (guarded([&] {
             describe(n.cropMat(fuse, 0, 40, 30, 10), out + 12);
             out[12] -= out[8], out[13] -= out[9];
           }) != REF_OK)
    threw |= 8;
  n.offset_x_ = saved_x, n.offset_y_ = saved_y;
  return threw;
}

int ref_geometry_batch(size_t count, const int *cols, const int *rows, const int *offset_x, const int *offset_y, int *out,
                       int *status) {
  for (size_t i = 0; i < count; ++i) {
    std::memset(out + 16 * i, 0, 16 * sizeof(int));
    status[i] = ref_geometry(cols[i], rows[i], offset_x[i], offset_y[i], out + 16 * i);
  }
  return REF_OK;
}

ref_node *ref_node_create(int offset_x, int offset_y, int have_offset_x, int have_offset_y) {
  ros::param_table().clear();
  if (have_offset_x) ros::param_table()["offset_x"] = offset_x;
  if (have_offset_y) ros::param_table()["offset_y"] = offset_y;
  ros::warnings().clear();
  ref_node *h = new ref_node;
  h->node = new DepthMapFusion();
  return h;
}

void ref_node_destroy(ref_node *h) {
  if (!h) return;
  delete h->node;
  delete h;
}

int ref_node_warnings(void) { return int(ros::warnings().size()); }

int ref_node_offsets(const ref_node *h, int out[2]) {
  if (!h) return REF_BAD_ARG;
  out[0] = h->node->offset_x_, out[1] = h->node->offset_y_;
  return REF_OK;
}

int ref_node_callback(ref_node *h, int which, const uint8_t *frame, size_t step, int cols, int rows, uint32_t seq,
                      const char *frame_id) {
  if (!h || !frame || cols <= 0 || rows <= 0 || step < size_t(cols) || which < 0 || which > 3) return REF_BAD_ARG;
  h->node->nh_.record->clear();
  sensor_msgs::ImagePtr msg = std::make_shared<sensor_msgs::Image>();
  msg->header.seq = seq, msg->header.stamp.sec = 1000 + seq, msg->header.stamp.nsec = 7 * seq;
  msg->header.frame_id = frame_id ? frame_id : "";
  msg->height = uint32_t(rows), msg->width = uint32_t(cols), msg->encoding = "mono8", msg->step = uint32_t(cols);
  msg->data.resize(size_t(cols) * size_t(rows));
  for (int i = 0; i < rows; ++i) std::memcpy(msg->data.data() + size_t(i) * size_t(cols), frame + size_t(i) * step, size_t(cols));
  const sensor_msgs::ImageConstPtr in = msg;
  return guarded([&] {
    switch (which) {
      case REF_DISPARITY_1: h->node->DisparityCb1(in); break;
      case REF_DISPARITY_2: h->node->DisparityCb2(in); break;
      case REF_MATCHING_SCORE_1: h->node->MatchingScoreCb1(in); break;
      default: h->node->MatchingScoreCb2(in); break;
    }
  });
}

int ref_node_published(const ref_node *h) { return h ? int(h->node->nh_.record->size()) : 0; }

int ref_node_topic(const ref_node *h, int index, ref_topic *out) {
  if (!h || !out || index < 0 || size_t(index) >= h->node->nh_.record->size()) return REF_BAD_ARG;
  const ros::Published &p = (*h->node->nh_.record)[size_t(index)];
  out->topic = p.topic.c_str(), out->encoding = p.msg.encoding.c_str(), out->frame_id = p.msg.header.frame_id.c_str();
  out->seq = p.msg.header.seq, out->width = p.msg.width, out->height = p.msg.height, out->step = p.msg.step;
  out->data = p.msg.data.data(), out->bytes = p.msg.data.size();
  return REF_OK;
}

}  // extern "C"
