// ros/depth_map_fusion_node.cpp -- the depth_map_fusion ROS node, source only (this image has no ROS / OpenCV /
// cv_bridge, so it cannot be built here; its logic is covered through the ROS-free instantiation in host/ and tests/,
// and the file itself is parsed and type-checked against declaration-only stubs by
// tests/test_fusion_session_cpu.py::test_ros_fusion_adaptor_parses -- a syntax check, nothing more).
//
// Same node name, subscribed and advertised topics, queue sizes and private parameters as the reference
// (src/depth_map_fusion_node.cpp:45-51, include/disparity_to_point_cloud/depth_map_fusion.hpp:96-125), so
// launch/depth_map_fusion.launch works unchanged.  cv_bridge::toCvCopy(msg, "mono8") stays the reference's call;
// everything behind it is the C-ABI session inside DepthMapFusionT.
#include <cv_bridge/cv_bridge.h>
#include <ros/param.h>
#include <ros/ros.h>
#include <sensor_msgs/Image.h>

#include <map>
#include <string>

#include "../host/depth_map_fusion_amd.hpp"

struct RosFusionMsgs {
  typedef sensor_msgs::Image Image;
  static d2pc::Mono8 prepare(const Image &msg, int /*median_ksize*/) {
    cv_bridge::CvImagePtr disparity = cv_bridge::toCvCopy(msg, "mono8");  // :47,:55,:65,:83
    d2pc::Mono8 out;
    out.width = disparity->image.cols;
    out.height = disparity->image.rows;
    out.pix.assign(disparity->image.datastart, disparity->image.dataend);  // continuous: freshly allocated
    return out;
  }
};

int main(int argc, char *argv[]) {
  ros::init(argc, argv, "depth_map_fusion");
  ros::NodeHandle nh("~");

  d2pc::FusionParamSource params;  // ~offset_x ~offset_y (hpp:119-124); a missing one warns inside the mirror
  for (const char *name : {"offset_x", "offset_y"}) {
    int v = 0;
    if (ros::param::get(std::string("~") + name, v)) params.values[name] = v;
  }
  int device = 0;
  nh.param("device_id", device, 0);  // rank-local GPU when several nodes share a host

  std::map<std::string, ros::Publisher> pubs;  // hpp:106-117
  for (const char *topic : {"/cropped_depth_1", "/cropped_depth_2", "/cropped_score_1", "/cropped_score_2", "/fused_depth_map",
                            "/combined_score", "/gradient"})
    pubs[topic] = nh.advertise<sensor_msgs::Image>(topic, 5);

  typedef d2pc::DepthMapFusionT<RosFusionMsgs> Node;
  Node node(
      params, [&](const char *topic, const sensor_msgs::Image &img) { pubs[topic].publish(img); }, device, -1,
      [](const std::string &text) { ROS_WARN("%s", text.c_str()); });
  // hpp:97-104
  ros::Subscriber d1 = nh.subscribe<sensor_msgs::Image>("/disparity_1", 1, [&](const sensor_msgs::ImageConstPtr &m) { node.DisparityCb1(m); });
  ros::Subscriber d2 = nh.subscribe<sensor_msgs::Image>("/disparity_2", 1, [&](const sensor_msgs::ImageConstPtr &m) { node.DisparityCb2(m); });
  ros::Subscriber s1 =
      nh.subscribe<sensor_msgs::Image>("/matching_score_1", 1, [&](const sensor_msgs::ImageConstPtr &m) { node.MatchingScoreCb1(m); });
  ros::Subscriber s2 =
      nh.subscribe<sensor_msgs::Image>("/matching_score_2", 1, [&](const sensor_msgs::ImageConstPtr &m) { node.MatchingScoreCb2(m); });
  (void)d1, (void)d2, (void)s1, (void)s2;
  ros::spin();  // single-threaded, as the reference (node.cpp:49)
  return 0;
}
