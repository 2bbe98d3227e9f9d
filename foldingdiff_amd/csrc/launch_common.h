// Host-only helpers shared by the launch wrappers at the end of the kernel sources and by api.hip's launch plan: the one
// definition of the CU count and the per-device LDS opt-in of kernels that need more than the default 64 KiB.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

namespace fdmi {

constexpr int kMaxDevices = 64;  // (a process may hold models on several GPUs: fd_create takes any device_id)

// compute units of the current device, cached per device; 256 (the MI355X) when the query fails
inline int cu_count() {
  static int cached[kMaxDevices] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
  if (cached[dev] == 0) {
    hipDeviceProp_t prop;
    cached[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  return cached[dev];
}

// x-grid of a persistent launch whose workgroups walk `items` (blockIdx.x, + gridDim.x, ...): one workgroup per CU and none without
// an item.  cap > 0 (option "debug_grid", tests only) lowers the workgroup count, so that a few items already give every workgroup
// several; it never raises it.
inline int persistent_grid(int items, int cap) {
  int grid = cu_count();
  if (cap > 0 && cap < grid) grid = cap;
  return items < grid ? items : grid;
}

// Opt-in of a kernel's instantiations to `bytes` of dynamic LDS, once per device (the attribute is per device).  One static
// instance per launch wrapper.  Tri-state: a runtime that refuses the opt-in must surface as a refused launch on every
// call, not as a silent no-op launch, and is not asked again.
struct LdsOptIn {
  int state[kMaxDevices] = {0};  // 0 unknown, 1 set, -1 refused
  bool operator()(std::initializer_list<const void*> kernels, int bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices) dev = 0;
    if (state[dev] == 0) {
      bool ok = true;
      for (const void* f : kernels) ok = ok && hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
      if (!ok) (void)hipGetLastError();  // (reported through the return value, not left behind as the thread's last error)
      state[dev] = ok ? 1 : -1;
    }
    return state[dev] > 0;
  }
};

}  // namespace fdmi
