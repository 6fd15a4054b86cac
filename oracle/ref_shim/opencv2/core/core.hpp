// Stand-in for the part of OpenCV that the reference's depth_map_fusion.cpp uses, written for this project's test
// oracle (oracle/ref.py compiles the reference against it; tests/README_reference.md).  8-bit, one or three channels, two dimensions; the semantics are
// OpenCV's where the reference depends on them:
//   * a Mat copy shares its pixels; mat(Rect) is a view that remembers where it lies in its parent (locateROI);
//   * mat(Rect) throws cv::Exception where OpenCV's CV_Assert(0 <= x, 0 <= width, x + width <= cols, ...) does;
//   * create() keeps the pixels of a Mat that already has the asked size and type;
//   * a + s * b saturates, and writes into the left-hand Mat's own pixels when that has the right size.
// cv::GaussianBlur, cv::Sobel and cv::threshold hold no arithmetic: they forward to hooks the loader installs.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

typedef unsigned char uchar;

#define CV_8U 0
#define CV_CN_SHIFT 3
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn)-1) << CV_CN_SHIFT))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)

namespace cv {

class Exception : public std::runtime_error {
 public:
  explicit Exception(const std::string &what) : std::runtime_error(what) {}
};

#define D2PC_SHIM_ASSERT(expr) \
  do {                         \
    if (!(expr)) throw cv::Exception(std::string("assertion failed: ") + #expr); \
  } while (0)
#define CV_Assert(expr) D2PC_SHIM_ASSERT(expr)

struct Size {
  int width = 0, height = 0;
  Size() {}
  Size(int w, int h) : width(w), height(h) {}
  bool operator==(const Size &o) const { return width == o.width && height == o.height; }
};

struct Point {
  int x = 0, y = 0;
};

struct Rect {
  int x = 0, y = 0, width = 0, height = 0;
  Rect() {}
  Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

struct Scalar {
  double val[4];
  Scalar(double a = 0, double b = 0, double c = 0, double d = 0) : val{a, b, c, d} {}
  static Scalar all(double v) { return Scalar(v, v, v, v); }
};

template <class T>
struct Point3_ {
  T x, y, z;
  Point3_() : x(0), y(0), z(0) {}
  Point3_(T a, T b, T c) : x(a), y(b), z(c) {}
};
typedef Point3_<float> Point3f;

inline uchar saturate_u8(double v) {
  const double r = std::nearbyint(v);  // the default rounding mode: half to even, as cvRound
  return r <= 0 ? 0 : r >= 255 ? 255 : uchar(r);
}

class Mat;
// alpha * a + beta * b, the only expression the reference forms (a + 2 * b)
struct MatExpr {
  const Mat *a = nullptr, *b = nullptr;
  double alpha = 1, beta = 1;
};

class Mat {
 public:
  int rows = 0, cols = 0;
  uchar *data = nullptr;
  size_t step = 0;

  Mat() {}
  Mat(int r, int c, int type) { create(r, c, type); }
  Mat(const MatExpr &e) { *this = e; }

  int type() const { return type_; }
  int channels() const { return (type_ >> CV_CN_SHIFT) + 1; }
  size_t elemSize() const { return size_t(channels()); }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  Size size() const { return Size(cols, rows); }

  void create(int r, int c, int type) {
    D2PC_SHIM_ASSERT(r >= 0 && c >= 0 && (type == CV_8UC1 || type == CV_8UC3));
    if (data && r == rows && c == cols && type == type_) return;
    type_ = type, rows = r, cols = c;
    step = size_t(c) * elemSize();
    buf_ = std::make_shared<std::vector<uchar>>(step * size_t(r) + 1);  // + 1: an empty image still has an address
    data = buf_->data();
    whole_rows_ = r, whole_cols_ = c, off_x_ = off_y_ = 0;
  }
  void create(Size s, int type) { create(s.height, s.width, type); }

  Mat operator()(const Rect &roi) const {
    D2PC_SHIM_ASSERT(0 <= roi.x && 0 <= roi.width && roi.x + roi.width <= cols && 0 <= roi.y && 0 <= roi.height &&
                     roi.y + roi.height <= rows);
    Mat m(*this);
    m.data = data + size_t(roi.y) * step + size_t(roi.x) * elemSize();
    m.rows = roi.height, m.cols = roi.width;
    m.off_x_ = off_x_ + roi.x, m.off_y_ = off_y_ + roi.y;
    return m;
  }

  // size of the allocation this Mat looks into, and where its first pixel lies there
  void locateROI(Size &whole, Point &ofs) const {
    whole = Size(whole_cols_, whole_rows_);
    ofs.x = off_x_, ofs.y = off_y_;
  }
  // the first pixel of the allocation (what locateROI's offset counts from)
  uchar *parent_data() const { return data - size_t(off_y_) * step - size_t(off_x_) * elemSize(); }

  template <class T>
  T &at(int i, int j) {
    return *reinterpret_cast<T *>(data + size_t(i) * step + size_t(j) * sizeof(T));
  }
  template <class T>
  const T &at(int i, int j) const {
    return *reinterpret_cast<const T *>(data + size_t(i) * step + size_t(j) * sizeof(T));
  }

  Mat clone() const {
    Mat m;
    m.create(rows, cols, type_);
    for (int i = 0; i < rows; ++i) std::memcpy(m.data + size_t(i) * m.step, data + size_t(i) * step, size_t(cols) * elemSize());
    return m;
  }

  Mat &operator=(const Scalar &s) {
    const int cn = channels();
    for (int i = 0; i < rows; ++i)
      for (int j = 0; j < cols; ++j)
        for (int c = 0; c < cn; ++c) data[size_t(i) * step + size_t(j) * cn + c] = saturate_u8(s.val[c]);
    return *this;
  }

  // MatExpr assignment: the destination is created (kept, when it already fits) and filled element by element, so a
  // destination that is also an operand is overwritten in place
  Mat &operator=(const MatExpr &e) {
    const Mat a = *e.a, b = *e.b;  // header copies keep the operands' pixels alive
    D2PC_SHIM_ASSERT(a.rows == b.rows && a.cols == b.cols && a.type_ == b.type_);
    create(a.rows, a.cols, a.type_);
    const size_t row = size_t(cols) * elemSize();
    for (int i = 0; i < rows; ++i)
      for (size_t j = 0; j < row; ++j)
        data[size_t(i) * step + j] = saturate_u8(e.alpha * a.data[size_t(i) * a.step + j] + e.beta * b.data[size_t(i) * b.step + j]);
    return *this;
  }

 private:
  int type_ = CV_8UC1;
  std::shared_ptr<std::vector<uchar>> buf_;
  int whole_rows_ = 0, whole_cols_ = 0, off_x_ = 0, off_y_ = 0;
};

// The operands must outlive the full expression: the reference only writes `x = a + 2 * b;`
inline MatExpr operator*(double s, const Mat &m) {
  MatExpr e;
  e.b = &m, e.beta = s;
  return e;
}
inline MatExpr operator+(const Mat &a, const MatExpr &scaled) {
  D2PC_SHIM_ASSERT(scaled.a == nullptr && scaled.b != nullptr);
  MatExpr e = scaled;
  e.a = &a, e.alpha = 1;
  return e;
}

inline void transpose(const Mat &src, Mat &dst) {
  D2PC_SHIM_ASSERT(src.type() == CV_8UC1);
  Mat out(src.cols, src.rows, CV_8UC1);
  for (int i = 0; i < src.rows; ++i)
    for (int j = 0; j < src.cols; ++j) out.at<uchar>(j, i) = src.at<uchar>(i, j);
  dst = out;
}

// flipCode > 0: around the vertical axis; 0: around the horizontal one; < 0: both
inline void flip(const Mat &src, Mat &dst, int flipCode) {
  D2PC_SHIM_ASSERT(src.type() == CV_8UC1);
  Mat out(src.rows, src.cols, CV_8UC1);
  for (int i = 0; i < src.rows; ++i)
    for (int j = 0; j < src.cols; ++j)
      out.at<uchar>(flipCode <= 0 ? src.rows - 1 - i : i, flipCode != 0 ? src.cols - 1 - j : j) = src.at<uchar>(i, j);
  dst = out;
}

}  // namespace cv
