// depth_map_fusion_amd.hpp -- host-side mirror of the reference's depth_map_fusion::DepthMapFusion
// (include/disparity_to_point_cloud/depth_map_fusion.hpp:63-155, src/depth_map_fusion.cpp:45-135) with every
// computing statement of the four callbacks replaced by ONE call into the C ABI's node session
// (d2pc_fusion_node_callback, include/d2pc.h).  Same callback names, same params (~offset_x ~offset_y, a missing one
// warns and stays 0), same seven topics in the reference's publishing order, header copied from the incoming
// message, "rgb8" for the coloured topics and "mono8" for the rest, so a node built from it drops into
// launch/depth_map_fusion.launch unchanged.
//
// Templated on a message policy `Msgs` { Image, static Mono8 prepare(const Image &, int median_ksize) } like
// Disparity2PCloudT: the ROS adaptor (ros/depth_map_fusion_node.cpp) instantiates it with sensor_msgs::Image +
// cv_bridge, the ROS-free harness with d2pc_shim::Image + image_prep.hpp.  cv_bridge::toCvCopy(msg, "mono8") stays on
// the host (prepare(msg, 0)).
//
// The session is created on the FIRST frame: the geometry comes from the message.  A frame the node cannot take -- an
// encoding cv_bridge refuses, another size than the session's, a device error -- is dropped with a warning and the
// node lives on (the policy tests/test_host_cpp.py pins for the point-cloud node).
#pragma once
#include <cstdio>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>

#include "../include/d2pc.h"
#include "image_prep.hpp"

namespace d2pc {

// nh_.getParam(name, int &) for the ROS-free build
struct FusionParamSource {
  std::map<std::string, int> values;
  bool getParam(const std::string &name, int &var) const {
    auto it = values.find(name);
    if (it == values.end()) return false;
    var = it->second;
    return true;
  }
};

template <class Msgs>
class DepthMapFusionT {
 public:
  typedef typename Msgs::Image Image;
  typedef std::function<void(const char *topic, const Image &)> Publisher;  // <topic>_pub_.publish
  typedef std::function<void(const std::string &)> Warn;                    // ROS_WARN

  int offset_x_ = 0;  // hpp:92-93
  int offset_y_ = 0;

 private:
  d2pc_ctx *ctx_ = nullptr;
  d2pc_fusion_node *node_ = nullptr;
  d2pc_fusion_node_geometry_t geo_{};
  int cols_ = 0, rows_ = 0, single_launch_ = -1;
  Publisher pub_;
  Warn warn_;
  size_t frames_dropped_ = 0;
  Image out_[D2PC_NODE_TOPICS];  // one message per topic, its data sized once

  static const char *topic_name(int id) {
    static const char *const names[D2PC_NODE_TOPICS] = {"/cropped_depth_1", "/cropped_depth_2", "/cropped_score_1", "/cropped_score_2",
                                                        "/fused_depth_map", "/combined_score", "/gradient"};
    return names[id];
  }

  void drop(const std::string &why) {
    ++frames_dropped_;
    warn_("depth_map_fusion: frame dropped: " + why);
  }

  bool make_session(int cols, int rows) {
    d2pc_fusion_node_config cfg;
    d2pc_fusion_node_config_init(&cfg);  // GRAD_FILTER (:159), crop 0/40/30/10 (:130)
    cfg.cols = cols, cfg.rows = rows, cfg.offset_x = offset_x_, cfg.offset_y = offset_y_;
    if (single_launch_ >= 0) cfg.single_launch = single_launch_;
    const int st = d2pc_fusion_node_create(ctx_, &cfg, &node_);
    if (st != D2PC_OK) {
      node_ = nullptr;
      drop(std::string("d2pc_fusion_node_create: ") + d2pc_status_string(st) + ": " + d2pc_last_error(ctx_));
      return false;
    }
    d2pc_fusion_node_geometry(&cfg, &geo_);
    cols_ = cols, rows_ = rows;
    for (int id = 0; id < D2PC_NODE_TOPICS; ++id) out_[id].data.resize(geo_.topic_bytes[id]);
    return true;
  }

  void callback(int which, const Image &msg) {
    Mono8 m;
    try {
      m = Msgs::prepare(msg, 0);  // cv_bridge::toCvCopy(*msg, "mono8") (:47,:55,:65,:83)
    } catch (const std::exception &e) {
      return drop(e.what());
    }
    if (!node_ && !make_session(m.width, m.height)) return;
    if (m.width != cols_ || m.height != rows_)
      return drop("a " + std::to_string(m.width) + "x" + std::to_string(m.height) + " frame in a session of " +
                  std::to_string(cols_) + "x" + std::to_string(rows_));
    d2pc_fusion_node_host_topics io;
    io = d2pc_fusion_node_host_topics();
    io.struct_size = sizeof io;
    for (int id = 0; id < D2PC_NODE_TOPICS; ++id) io.data[id] = out_[id].data.data(), io.capacity[id] = out_[id].data.size();
    const int st = d2pc_fusion_node_callback(node_, which, m.pix.data(), size_t(m.width), &io);
    if (st != D2PC_OK) return drop(std::string(d2pc_status_string(st)) + ": " + d2pc_last_error(ctx_));
    // the reference's order: DisparityCb2 publishes /cropped_depth_2 (:59), then publishFusedDepthMap /combined_score
    // (:126), /gradient (:132), /fused_depth_map (:136)
    static const int order[D2PC_NODE_TOPICS] = {D2PC_TOPIC_CROPPED_DEPTH_1, D2PC_TOPIC_CROPPED_DEPTH_2, D2PC_TOPIC_CROPPED_SCORE_1,
                                                D2PC_TOPIC_CROPPED_SCORE_2, D2PC_TOPIC_COMBINED_SCORE, D2PC_TOPIC_GRADIENT,
                                                D2PC_TOPIC_FUSED_DEPTH_MAP};
    for (int id : order) {
      if (!((io.published >> id) & 1u)) continue;
      Image &o = out_[id];
      o.header = msg.header;  // publishWithColor: out_msg.header = msg->header (:282,:297)
      o.height = uint32_t(io.height[id]);
      o.width = uint32_t(io.width[id]);
      o.encoding = io.channels[id] == 3 ? "rgb8" : "mono8";
      o.is_bigendian = 0;
      o.step = uint32_t(io.width[id] * io.channels[id]);
      pub_(topic_name(id), o);
    }
  }

 public:
  // hpp:96-125.  single_launch: -1 = the library's default, else d2pc_fusion_node_config::single_launch
  DepthMapFusionT(const FusionParamSource &nh, Publisher pub, int device_id = 0, int single_launch = -1, Warn warn = Warn())
      : single_launch_(single_launch), pub_(std::move(pub)), warn_(std::move(warn)) {
    if (!warn_) warn_ = [](const std::string &s) { fprintf(stderr, "[ WARN] %s\n", s.c_str()); };
    if (!nh.getParam("offset_x", offset_x_)) warn_("Failed to load parameter offset_x");  // :119-124
    if (!nh.getParam("offset_y", offset_y_)) warn_("Failed to load parameter offset_y");
    if (d2pc_abi_version() != D2PC_ABI_VERSION)
      throw std::runtime_error("libd2pc.so has ABI version " + std::to_string(d2pc_abi_version()) + ", this node was built against " +
                               std::to_string(D2PC_ABI_VERSION));
    d2pc_config cfg;
    d2pc_config_init(&cfg);
    cfg.device_id = device_id;
    const int st = d2pc_create(&cfg, &ctx_);
    if (st != D2PC_OK) throw std::runtime_error(std::string("d2pc_create: ") + d2pc_status_string(st));
  }
  ~DepthMapFusionT() {
    if (node_) d2pc_fusion_node_destroy(node_);
    if (ctx_) d2pc_destroy(ctx_);
  }
  DepthMapFusionT(const DepthMapFusionT &) = delete;
  DepthMapFusionT &operator=(const DepthMapFusionT &) = delete;

  size_t frames_dropped() const { return frames_dropped_; }
  d2pc_fusion_node *session() { return node_; }  // null until the first frame

  void DisparityCb1(const typename Image::ConstPtr &msg) { callback(D2PC_NODE_DISPARITY_1, *msg); }
  void DisparityCb2(const typename Image::ConstPtr &msg) { callback(D2PC_NODE_DISPARITY_2, *msg); }
  void MatchingScoreCb1(const typename Image::ConstPtr &msg) { callback(D2PC_NODE_MATCHING_SCORE_1, *msg); }
  void MatchingScoreCb2(const typename Image::ConstPtr &msg) { callback(D2PC_NODE_MATCHING_SCORE_2, *msg); }
};

}  // namespace d2pc
