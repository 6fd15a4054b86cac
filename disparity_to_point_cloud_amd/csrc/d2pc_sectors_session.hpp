// d2pc_sectors_session.hpp -- what the sessions of include/d2pc_sectors.h (d2pc_sectors_capi.hip,
// d2pc_sectors_memory_capi.hip, d2pc_sectors_steer_capi.hip) share on the host and need the HIP runtime for: selecting the
// session's device, the device-id check, the boundary tables in device memory (the grid's and the memory's; the steer
// uploads its own reach tables) and a session's error string.  (The plan headers stay free of HIP.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <vector>

#include "d2pc_sectors_plan.hpp"

namespace d2pc {
namespace sectors {

struct DeviceGuard {   // selects the session's device for a scope (as the contexts of libd2pc.so do)
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

inline bool device_exists(int device_id) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess && device_id >= 0 && device_id < n_dev) return true;
  (void)hipGetLastError();
  return false;
}

// half x (c, s), then plan.elev x (ce, se), interleaved, allocated and copied to the selected device
inline hipError_t upload_table(const d2pc_sectors_config &cfg, const Plan &p, float **d_table) {
  const size_t pairs = size_t(p.half) + size_t(p.elev);
  std::vector<float> table(pairs * 2), cs(pairs), sn(pairs);
  fill_table(cfg, cs.data(), sn.data());
  if (p.elev) fill_elevation_table(cfg, cs.data() + p.half, sn.data() + p.half);
  for (size_t j = 0; j < pairs; ++j) table[2 * j] = cs[j], table[2 * j + 1] = sn[j];
  const hipError_t e = hipMalloc(reinterpret_cast<void **>(d_table), table.size() * sizeof(float));
  return e != hipSuccess ? e : hipMemcpy(*d_table, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice);
}

// `status`, with its reason in the session's error string
template <size_t kLen>
int fail(char (&err)[kLen], int status, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err, kLen, fmt, ap);
  va_end(ap);
  return status;
}

}  // namespace sectors
}  // namespace d2pc
