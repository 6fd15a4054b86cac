// Stand-in: the plain message struct the reference's callbacks take and publish (fields of sensor_msgs/Image).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace ros {
struct Time {
  uint32_t sec = 0, nsec = 0;
};
}  // namespace ros

namespace std_msgs {
struct Header {
  uint32_t seq = 0;
  ros::Time stamp;
  std::string frame_id;
};
}  // namespace std_msgs

namespace sensor_msgs {
struct Image {
  std_msgs::Header header;
  uint32_t height = 0, width = 0;
  std::string encoding;
  uint8_t is_bigendian = 0;
  uint32_t step = 0;
  std::vector<uint8_t> data;
  typedef std::shared_ptr<Image> Ptr;
  typedef std::shared_ptr<const Image> ConstPtr;
};
typedef Image::Ptr ImagePtr;
typedef Image::ConstPtr ImageConstPtr;
}  // namespace sensor_msgs
