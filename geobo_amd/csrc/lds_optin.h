// lds_optin.h -- the library's one piece of process-global state (include/geobo_hip.h, conventions), in one place.
// A kernel with more than 64 KiB of dynamic LDS needs hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per DEVICE.  Its launcher
// keeps `static std::atomic<uint64_t> attr_done{0};` -- ONE MASK PER KERNEL, bit d = "issued on device d" -- and passes it here before
// the launch.  (The mask is the caller's: a static in a template on the kernel's pointer TYPE would be shared by every kernel of one
// signature, and the second would never get its attribute.)  Idempotent, lock free, never cleared.
#ifndef GEOBO_LDS_OPTIN_H
#define GEOBO_LDS_OPTIN_H

#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "geobo_hip.h"

namespace {

template <class Kern>
int ensure_lds_attr(std::atomic<uint64_t>& done, Kern kern, size_t lds) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return GEOBO_E_LAUNCH;
  if ((done.load(std::memory_order_acquire) >> dev) & 1) return GEOBO_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return GEOBO_E_LAUNCH;
  done.fetch_or((uint64_t)1 << dev, std::memory_order_release);
  return GEOBO_OK;
}

}  // namespace

#endif
