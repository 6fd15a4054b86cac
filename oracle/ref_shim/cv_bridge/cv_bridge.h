// Stand-in for cv_bridge: CvImage with both toImageMsg forms, and toCvCopy(msg, "mono8") as a deep copy of a mono8
// message (any other conversion throws: the harness only feeds mono8).
#pragma once
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "../opencv2/core/core.hpp"
#include "../sensor_msgs/Image.h"

namespace cv_bridge {

class Exception : public std::runtime_error {
 public:
  explicit Exception(const std::string &what) : std::runtime_error(what) {}
};

class CvImage {
 public:
  std_msgs::Header header;
  std::string encoding;
  cv::Mat image;

  // rows packed: step = width x channels, whatever the Mat's own step is
  void toImageMsg(sensor_msgs::Image &msg) const {
    msg.header = header;
    msg.height = uint32_t(image.rows), msg.width = uint32_t(image.cols);
    msg.encoding = encoding;
    msg.is_bigendian = 0;
    const size_t row = size_t(image.cols) * image.elemSize();
    msg.step = uint32_t(row);
    msg.data.resize(row * size_t(image.rows));
    for (int i = 0; i < image.rows; ++i) std::memcpy(msg.data.data() + size_t(i) * row, image.data + size_t(i) * image.step, row);
  }
  sensor_msgs::ImagePtr toImageMsg() const {
    sensor_msgs::ImagePtr msg = std::make_shared<sensor_msgs::Image>();
    toImageMsg(*msg);
    return msg;
  }
};
typedef std::shared_ptr<CvImage> CvImagePtr;

inline CvImagePtr toCvCopy(const sensor_msgs::Image &msg, const std::string &encoding = std::string()) {
  if (msg.encoding != "mono8" || (!encoding.empty() && encoding != "mono8"))
    throw Exception("the stand-in converts mono8 to mono8 only, not " + msg.encoding + " to " + encoding);
  if (msg.step < msg.width || msg.data.size() < size_t(msg.step) * msg.height) throw Exception("image message too short");
  CvImagePtr out = std::make_shared<CvImage>();
  out->header = msg.header;
  out->encoding = "mono8";
  out->image.create(int(msg.height), int(msg.width), CV_8UC1);
  for (uint32_t i = 0; i < msg.height; ++i)
    std::memcpy(out->image.data + size_t(i) * out->image.step, msg.data.data() + size_t(i) * msg.step, msg.width);
  return out;
}
inline CvImagePtr toCvCopy(const sensor_msgs::ImageConstPtr &msg, const std::string &encoding = std::string()) {
  return toCvCopy(*msg, encoding);
}

}  // namespace cv_bridge
