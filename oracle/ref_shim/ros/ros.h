// Stand-in for roscpp: a NodeHandle whose parameters come from a table the harness fills, whose subscriptions do
// nothing (the harness calls the callbacks itself) and whose publishers record every message, in publishing order.
#pragma once
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../sensor_msgs/Image.h"

namespace ros {

struct Published {
  std::string topic;
  sensor_msgs::Image msg;
};
typedef std::vector<Published> Record;

// nh_.getParam(name, int &): filled by the harness before the node is constructed
inline std::map<std::string, int> &param_table() {
  static std::map<std::string, int> table;
  return table;
}
// what ROS_WARN printed since the harness last cleared it
inline std::vector<std::string> &warnings() {
  static std::vector<std::string> list;
  return list;
}

class Subscriber {};

class Publisher {
 public:
  Publisher() {}
  Publisher(const std::string &topic, std::shared_ptr<Record> record) : topic_(topic), record_(std::move(record)) {}
  void publish(const sensor_msgs::Image &msg) const {
    if (record_) record_->push_back(Published{topic_, msg});
  }
  void publish(const sensor_msgs::ImagePtr &msg) const { publish(*msg); }
  void publish(const sensor_msgs::ImageConstPtr &msg) const { publish(*msg); }

 private:
  std::string topic_;
  std::shared_ptr<Record> record_;
};

class NodeHandle {
 public:
  explicit NodeHandle(const std::string &ns = std::string()) : ns_(ns), record(std::make_shared<Record>()) {}

  template <class M, class T>
  Subscriber subscribe(const std::string &, uint32_t, void (T::*)(const std::shared_ptr<const M> &), T *) {
    return Subscriber();
  }
  template <class M>
  Publisher advertise(const std::string &topic, uint32_t) {
    return Publisher(topic, record);
  }
  bool getParam(const std::string &name, int &value) const {
    auto it = param_table().find(name);
    if (it == param_table().end()) return false;
    value = it->second;
    return true;
  }

 private:
  std::string ns_;

 public:
  std::shared_ptr<Record> record;  // every message of every publisher this handle advertised
};

}  // namespace ros

#define ROS_WARN(...)                          \
  do {                                         \
    char ros_warn_text[512];                   \
    std::snprintf(ros_warn_text, sizeof ros_warn_text, __VA_ARGS__); \
    ros::warnings().push_back(ros_warn_text);  \
  } while (0)
