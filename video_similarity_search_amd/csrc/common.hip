// Library-wide entry points: version, error string, device check; the per-device launch state every launcher shares.
#include "common.h"
#include <stdarg.h>
#include <string.h>
#include <map>
#include <mutex>
#include <utility>

static thread_local char g_err[512] = "";

void slic_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int slic_version(void) { return (0 << 16) | (1 << 8) | 0; }

extern "C" const char* slic_last_error(void) { return g_err; }

extern "C" int slic_device_check(void) {
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    slic_set_error("no HIP device visible");
    return SLIC_ENODEV;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    slic_set_error("device is %s, this library is built for gfx950 only", prop.gcnArchName);
    return SLIC_ENODEV;
  }
  return SLIC_OK;
}

// What launchers need to know about a device, keyed by its ordinal: one lock, a few dozen entries.
static std::mutex g_dev_mu;
static std::map<std::pair<int, const void*>, size_t> g_lds_limit;   // (device, kernel) -> largest dynamic-LDS limit set
static std::map<int, int> g_cus;                                    // device -> compute units

int slic_lds_limit(const void* kernel, size_t bytes) {
  if (bytes > 160 * 1024) {                                         // more than a compute unit has: no launch could use it
    slic_set_error("slic_lds_limit: %zu bytes of dynamic LDS", bytes);
    return SLIC_EHIP;
  }
  int dev = 0;
  SLIC_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_dev_mu);
  const auto key = std::make_pair(dev, kernel);
  const auto it = g_lds_limit.find(key);
  if (it != g_lds_limit.end() && bytes <= it->second) return SLIC_OK;
  SLIC_HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  g_lds_limit[key] = bytes;                                         // recorded only once the runtime has accepted it
  return SLIC_OK;
}

int slic_device_cus(void) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  std::lock_guard<std::mutex> lock(g_dev_mu);
  auto it = g_cus.find(dev);
  if (it != g_cus.end()) return it->second;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); return 0; }
  g_cus[dev] = cus;
  return cus;
}
