// Library-level entry points of libbevf_hip.so: version, per-thread error text and the dynamic-LDS opt-in table.
#include "common.h"

#include <map>
#include <mutex>
#include <utility>

static thread_local char g_err[512] = "";

void bevf_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// Dynamic LDS granted so far, per (kernel, device ordinal): the attribute lives in the current device's copy of the kernel.
static std::mutex g_lds_mutex;
static std::map<std::pair<const void*, int>, size_t> g_lds_granted;

int bevf_grant_lds(const char* entry, const void* kernel, size_t lds_bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) {
    bevf_set_error("%s: hipGetDevice failed: %s", entry, hipGetErrorString(e));
    return BEVF_ERR_LAUNCH;
  }
  std::lock_guard<std::mutex> lock(g_lds_mutex);
  const auto key = std::make_pair(kernel, dev);
  const auto it = g_lds_granted.find(key);
  if (it != g_lds_granted.end() && it->second >= lds_bytes) return BEVF_OK;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();   // reported here: do not leave it for the next launch check to find
    bevf_set_error("%s: cannot raise dynamic LDS to %zu bytes: %s", entry, lds_bytes, hipGetErrorString(e));
    return BEVF_ERR_LAUNCH;
  }
  g_lds_granted[key] = lds_bytes;
  return BEVF_OK;
}

extern "C" int bevf_version(void) { return 220; }  // 0.2.2: round 2 -- decode / conv descriptors grew; Winograd forward + weight gradient, fused stem + pool, fused PointNet front entries
extern "C" const char* bevf_last_error(void) { return g_err; }
