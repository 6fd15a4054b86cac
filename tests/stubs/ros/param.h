// SYNTAX-CHECK STUB (see tests/stubs/README.md): declarations only, never linked or run.
#pragma once
#include <ros/ros.h>
#define ROS_WARN(...) ::ros::stub_warn(__VA_ARGS__)
namespace ros {
void stub_warn(const char *fmt, ...);
namespace param {
bool get(const std::string &key, int &v);
}  // namespace param
}  // namespace ros
