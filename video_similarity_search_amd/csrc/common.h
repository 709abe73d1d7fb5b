// Shared helpers for libslic_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/slic_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

void slic_set_error(const char* fmt, ...);

#define SLIC_REQUIRE(cond, ...)                 \
  do {                                          \
    if (!(cond)) {                              \
      slic_set_error(__VA_ARGS__);              \
      return SLIC_EINVAL;                       \
    }                                           \
  } while (0)

#define SLIC_HIP_CHECK(expr)                                                        \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      slic_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return SLIC_EHIP;                                                             \
    }                                                                               \
  } while (0)

#define SLIC_LAUNCH_CHECK() SLIC_HIP_CHECK(hipGetLastError())

// Raise `kernel`'s dynamic-LDS limit on the current device to at least `bytes`.  The limit is remembered per (device, kernel)
// and only ever raised, so call it before every launch with the size about to be used.  SLIC_OK or SLIC_EHIP (+ slic_last_error).
int slic_lds_limit(const void* kernel, size_t bytes);
// compute units of the current device; 0 when no device answers
int slic_device_cus(void);

#define SLIC_LDS_LIMIT(kernel, bytes)                                  \
  do {                                                                 \
    int _rc = slic_lds_limit((const void*)(kernel), (size_t)(bytes));  \
    if (_rc != SLIC_OK) return _rc;                                    \
  } while (0)

static inline hipStream_t S_(void* s) { return (hipStream_t)s; }

static inline size_t slic_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int64_t slic_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// carve consecutive 256-byte aligned regions out of a caller workspace
struct SlicCarver {
  char* p;
  size_t off;
  explicit SlicCarver(void* base) : p((char*)base), off(0) {}
  template <typename T>
  T* take(size_t n) {
    T* r = (T*)(p + off);
    off += slic_align_up(n * sizeof(T), 256);
    return r;
  }
};
