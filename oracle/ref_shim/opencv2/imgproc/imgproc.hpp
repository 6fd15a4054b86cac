// Stand-in for the OpenCV image filters the reference's depth_map_fusion.cpp calls.
//   cv::medianBlur           an order statistic written here: replicated border that never looks outside the Mat it
//                            was given (a view's parent is not read), safe when src and dst are one Mat.
//   cv::GaussianBlur/Sobel/threshold
//                            no arithmetic here: they describe their operands and forward to a hook
//                            (ref_filter_hooks).  A call without a hook throws, which the harness reports as a status.
//   cv::applyColorMap        declared because the reference names it; aborts when reached (it never is: the node only
//                            uses its own two colourings).
#pragma once
#include <cstdio>
#include <cstdlib>

#include "../core/core.hpp"

extern "C" {
// One operand of a filter: `rows` x `cols` 8-bit pixels `step` bytes apart, lying at (x, y) of an allocation of
// parent_rows x parent_cols pixels that starts at `parent` (the same `step`).  A whole Mat has x = y = 0.
typedef struct ref_view {
  unsigned char *data;
  unsigned long long step;
  int rows, cols;
  unsigned char *parent;
  int parent_rows, parent_cols, x, y;
} ref_view;

// Each hook returns 0 on success.  src and dst may describe the same pixels (the reference filters in place).
typedef int (*ref_gaussian_hook)(const ref_view *src, const ref_view *dst, int ksize_x, int ksize_y, double sigma);
typedef int (*ref_sobel_hook)(const ref_view *src, const ref_view *dst, int dx, int dy, int ksize, double scale);
typedef int (*ref_threshold_hook)(const ref_view *src, const ref_view *dst, double thresh, double maxval, int type);

typedef struct ref_filter_hooks {
  ref_gaussian_hook gaussian;
  ref_sobel_hook sobel;
  ref_threshold_hook threshold;
} ref_filter_hooks;

// defined once, in the harness
extern ref_filter_hooks ref_hooks;
}

namespace cv {

class HookMissing : public Exception {
 public:
  explicit HookMissing(const std::string &what) : Exception(what) {}
};

inline ref_view describe_view(const Mat &m) {
  Size whole;
  Point ofs;
  m.locateROI(whole, ofs);
  ref_view v;
  v.data = m.data, v.step = m.step, v.rows = m.rows, v.cols = m.cols;
  v.parent = m.parent_data(), v.parent_rows = whole.height, v.parent_cols = whole.width, v.x = ofs.x, v.y = ofs.y;
  return v;
}

// dst.create(src.size(), src.type()) as every OpenCV filter does: a dst that already fits keeps its pixels
inline void prepare_filter(const Mat &src, Mat &dst) {
  D2PC_SHIM_ASSERT(src.type() == CV_8UC1 && !src.empty());
  dst.create(src.size(), src.type());
}

inline void GaussianBlur(const Mat &src_, Mat &dst, Size ksize, double sigma) {
  const Mat src = src_;
  prepare_filter(src, dst);
  if (!ref_hooks.gaussian) throw HookMissing("cv::GaussianBlur: no hook installed");
  const ref_view s = describe_view(src), d = describe_view(dst);
  if (ref_hooks.gaussian(&s, &d, ksize.width, ksize.height, sigma) != 0) throw Exception("cv::GaussianBlur: the hook failed");
}

inline void Sobel(const Mat &src_, Mat &dst, int ddepth, int dx, int dy, int ksize, double scale) {
  const Mat src = src_;
  D2PC_SHIM_ASSERT(ddepth == -1);
  prepare_filter(src, dst);
  if (!ref_hooks.sobel) throw HookMissing("cv::Sobel: no hook installed");
  const ref_view s = describe_view(src), d = describe_view(dst);
  if (ref_hooks.sobel(&s, &d, dx, dy, ksize, scale) != 0) throw Exception("cv::Sobel: the hook failed");
}

inline double threshold(const Mat &src_, Mat &dst, double thresh, double maxval, int type) {
  const Mat src = src_;
  prepare_filter(src, dst);
  if (!ref_hooks.threshold) throw HookMissing("cv::threshold: no hook installed");
  const ref_view s = describe_view(src), d = describe_view(dst);
  if (ref_hooks.threshold(&s, &d, thresh, maxval, type) != 0) throw Exception("cv::threshold: the hook failed");
  return thresh;
}

inline void medianBlur(const Mat &src_, Mat &dst, int ksize) {
  D2PC_SHIM_ASSERT(src_.type() == CV_8UC1 && ksize >= 3 && ksize % 2 == 1 && ksize <= 7);
  const Mat src = src_.clone();  // src may be dst
  dst.create(src.size(), src.type());
  const int r = ksize / 2, count = ksize * ksize;
  uchar window[49];
  for (int i = 0; i < src.rows; ++i)
    for (int j = 0; j < src.cols; ++j) {
      int k = 0;
      for (int di = -r; di <= r; ++di)
        for (int dj = -r; dj <= r; ++dj)
          window[k++] = src.at<uchar>(std::min(std::max(i + di, 0), src.rows - 1), std::min(std::max(j + dj, 0), src.cols - 1));
      std::nth_element(window, window + count / 2, window + count);
      dst.at<uchar>(i, j) = window[count / 2];
    }
}

inline void applyColorMap(const Mat &, Mat &, int) {
  std::fprintf(stderr, "cv::applyColorMap is not part of the stand-in\n");
  std::abort();
}

}  // namespace cv
