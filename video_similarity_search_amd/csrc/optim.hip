// Multi-tensor parameter updates (optim.py): SGD, Adam and the MoCo key-encoder EMA, each as ONE launch over every tensor of every
// parameter group of one optimizer.  A pure stream: momentum SGD reads p, g, buf and writes p, buf (five streams of 4 bytes per
// element), Adam reads p, g, m, v and writes p, m, v (seven), the EMA reads k, q and writes k (three).
//
// Two tables, both built on the host (optim.py: build_chunk_map, build_descriptors):
//   map   int32 [n_items][2]   (tensor, chunk within the tensor); chunk c of a tensor is its elements [c * CHUNK, (c + 1) * CHUNK) ∩ [0, n),
//                              so no item spans two tensors.  Static for a parameter set: uploaded once.
//   desc  MtDesc [n_tensors]   128 bytes per tensor: pointers, length, flags, hyper-parameters as doubles.  Uploaded when it changed.
// The per-step upload is therefore O(tensors) (8 KB for R3D-18's 62 tensors), never O(parameters / CHUNK).
//
// Element offsets are 64-bit (chunk * CHUNK in int64): a tensor of more than 2^31 elements does not wrap.
//
// A workgroup takes items blockIdx.x, blockIdx.x + gridDim.x, ...  Where the tensor's SLIC_MT_VEC flag is set (every pointer the
// operation uses is 16-byte aligned; CHUNK is a multiple of 4, so every chunk start is too) a thread moves float4s, all loads of an
// item issued before the first use: 4 float4 per stream per thread, 48 KiB (SGD) to 64 KiB (Adam) of loads in flight per workgroup.
// The last len % 4 elements of a tensor and every item of a tensor without the flag (a gradient that is a view into a flat bucket,
// a flattened parameter: 4-byte aligned only) go element by element.  Nothing is read or written past element n - 1.
// A map entry that names no tensor or no chunk of its tensor is skipped, so no map can make the kernel leave a tensor; the
// descriptors are validated on their host copy before every launch.
//
// Rounding: this file is compiled with -ffp-contract=off (FLAGS_optim) and spells every fused multiply-add as fmaf, so what is
// written below is what runs: one rounding per a * b + c of the update chains (g + wd * p, mom * buf + ..., p - lr * u, ...).
// Hyper-parameters arrive as doubles and are rounded to fp32 once, here, as torch rounds its Python scalars.  sqrt and divide are
// correctly rounded (hipcc's default for fp32).
//
//   SGD   h[0] lr, h[1] momentum, h[2] 1 - dampening, h[3] weight_decay; SLIC_MT_NESTEROV, SLIC_MT_FIRST (or all_first: every tensor's first step)
//         g' = g + wd p;  buf = first ? g' : mom buf + (1 - damp) g';  p -= lr (nesterov ? g' + mom buf : buf);  mom == 0: p -= lr g', s1 unused
//   Adam  h[0] lr / bc1, h[1] 1 - beta1, h[2] beta2, h[3] 1 - beta2, h[4] eps, h[5] weight_decay, h[6] sqrt(bc2)     (bc = 1 - beta^step, host, double)
//         g' = g + wd p;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
//   EMA   h[0] m, h[1] 1 - m:  p = p m + g (1 - m)        (p: the key parameter, g: the query parameter)
#include <math.h>
#include <string.h>
#include "common.h"

#define MT_THREADS 256
#define MT_CHUNK 4096
#define MT_VPT (MT_CHUNK / 4 / MT_THREADS)      // float4 per thread per stream per item
#define MT_BLOCKS_PER_CU 8
enum { MT_SGD = 0, MT_ADAM = 1, MT_EMA = 2 };

struct MtDesc {
  uint64_t p, g, s1, s2;
  int64_t n;
  int32_t flags, pad;
  double h[SLIC_MT_HYPER];
};
static_assert(sizeof(MtDesc) == SLIC_MT_DESC_BYTES, "descriptor layout is part of the ABI");
static_assert(MT_CHUNK % (4 * MT_THREADS) == 0, "a chunk is a whole number of float4 passes");

// the table's addresses are device memory: say so, and the loads and stores are global_*, not flat_*
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

struct MtHyper {
  float a, b, c, d, e, f, g;
  bool wd, mom, nesterov, first;
};

template <int OP>
__device__ __forceinline__ MtHyper mt_hyper(const MtDesc& d, int all_first) {
  MtHyper h = {};
  if constexpr (OP == MT_SGD) {
    h.a = (float)d.h[0]; h.b = (float)d.h[1]; h.c = (float)d.h[2]; h.d = (float)d.h[3];
    h.wd = d.h[3] != 0.0;
    h.mom = d.h[1] != 0.0;
    h.nesterov = d.flags & SLIC_MT_NESTEROV;
    h.first = all_first || (d.flags & SLIC_MT_FIRST);
  } else if constexpr (OP == MT_ADAM) {
    h.a = (float)d.h[0]; h.b = (float)d.h[1]; h.c = (float)d.h[2]; h.d = (float)d.h[3]; h.e = (float)d.h[4]; h.f = (float)d.h[5];
    h.g = (float)d.h[6];
    h.wd = d.h[5] != 0.0;
  } else {
    h.a = (float)d.h[0]; h.b = (float)d.h[1];
  }
  return h;
}

// one element: p, s1, s2 updated in place (s1: momentum_buffer / exp_avg, s2: exp_avg_sq)
template <int OP>
__device__ __forceinline__ void mt_update(const MtHyper& h, float& p, float g, float& s1, float& s2) {
  if constexpr (OP == MT_SGD) {
    if (h.wd) g = fmaf(h.d, p, g);
    float u = g;
    if (h.mom) {
      s1 = h.first ? g : fmaf(h.b, s1, h.c * g);
      u = h.nesterov ? fmaf(h.b, s1, g) : s1;
    }
    p = fmaf(-h.a, u, p);
  } else if constexpr (OP == MT_ADAM) {
    if (h.wd) g = fmaf(h.f, p, g);
    s1 = fmaf(h.b, g - s1, s1);
    s2 = fmaf(h.d * g, g, h.c * s2);
    const float denom = sqrtf(s2) / h.g + h.e;
    p = fmaf(-h.a, s1 / denom, p);
  } else {
    p = fmaf(p, h.a, g * h.b);
  }
}

template <int OP>
__global__ __launch_bounds__(MT_THREADS) void mt_kernel(const int2* __restrict__ map, int n_items, const MtDesc* __restrict__ desc, int n_tensors,
                                                       int all_first) {
  constexpr bool S1 = OP != MT_EMA, S2 = OP == MT_ADAM;
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int2 it = map[item];
    if (it.x < 0 || it.x >= n_tensors || it.y < 0) continue;
    const MtDesc& d = desc[it.x];
    const int64_t off = (int64_t)it.y * MT_CHUNK;
    if (off >= d.n) continue;
    const int len = (int)(d.n - off < (int64_t)MT_CHUNK ? d.n - off : (int64_t)MT_CHUNK);
    const MtHyper h = mt_hyper<OP>(d, all_first);
    const bool use1 = S1 && (OP == MT_ADAM || h.mom);          // SGD without momentum has no buffer
    gfloat* p = (gfloat*)d.p + off;
    const gfloat* g = (const gfloat*)d.g + off;
    gfloat* s1 = use1 ? (gfloat*)d.s1 + off : nullptr;
    gfloat* s2 = S2 ? (gfloat*)d.s2 + off : nullptr;
    int done = 0;                                              // elements [0, done) of the item went as float4
    if (d.flags & SLIC_MT_VEC) {
      const int nv = len >> 2;
      done = nv << 2;
      f32x4 P[MT_VPT], G[MT_VPT], A[MT_VPT] = {}, B[MT_VPT] = {};
#pragma unroll
      for (int k = 0; k < MT_VPT; ++k) {
        const int i = threadIdx.x + k * MT_THREADS;
        if (i < nv) {
          P[k] = ((const gf32x4*)p)[i];
          G[k] = ((const gf32x4*)g)[i];
          // a first SGD step defines the buffer: it is not read
          if (use1 && !(OP == MT_SGD && h.first)) A[k] = ((const gf32x4*)s1)[i];
          if (S2) B[k] = ((const gf32x4*)s2)[i];
        }
      }
#pragma unroll
      for (int k = 0; k < MT_VPT; ++k) {
        const int i = threadIdx.x + k * MT_THREADS;
        if (i < nv) {
          f32x4 a = A[k], b = B[k], q = P[k];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float pj = q[j], aj = a[j], bj = b[j];
            mt_update<OP>(h, pj, G[k][j], aj, bj);
            q[j] = pj; a[j] = aj; b[j] = bj;
          }
          ((gf32x4*)p)[i] = q;
          if (use1) ((gf32x4*)s1)[i] = a;
          if (S2) ((gf32x4*)s2)[i] = b;
        }
      }
    }
    for (int i = done + threadIdx.x; i < len; i += MT_THREADS) {
      float pj = p[i], aj = 0.f, bj = 0.f;
      if (use1 && !(OP == MT_SGD && h.first)) aj = s1[i];
      if (S2) bj = s2[i];
      mt_update<OP>(h, pj, g[i], aj, bj);
      p[i] = pj;
      if (use1) s1[i] = aj;
      if (S2) s2[i] = bj;
    }
  }
}

// every descriptor names memory the kernel may touch as it will touch it: fp32-aligned pointers, the state the operation needs, a
// vector flag only over 16-byte aligned pointers, finite hyper-parameters
static int mt_validate(const char* who, int op, const void* desc_host, int n_tensors) {
  for (int t = 0; t < n_tensors; ++t) {
    MtDesc d;
    memcpy(&d, (const char*)desc_host + (size_t)t * sizeof(MtDesc), sizeof(MtDesc));
    SLIC_REQUIRE(d.n > 0 && d.n <= (int64_t)INT32_MAX * MT_CHUNK, "%s: tensor %d: length %lld", who, t, (long long)d.n);
    SLIC_REQUIRE(d.p && d.g, "%s: tensor %d: NULL parameter or gradient", who, t);
    const bool need1 = op == MT_ADAM || (op == MT_SGD && d.h[1] != 0.0), need2 = op == MT_ADAM;
    SLIC_REQUIRE(!need1 || d.s1, "%s: tensor %d: NULL %s", who, t, op == MT_ADAM ? "exp_avg" : "momentum_buffer");
    SLIC_REQUIRE(!need2 || d.s2, "%s: tensor %d: NULL exp_avg_sq", who, t);
    const uint64_t all = d.p | d.g | (need1 ? d.s1 : 0) | (need2 ? d.s2 : 0);
    SLIC_REQUIRE((all & 3) == 0, "%s: tensor %d: a pointer is not 4-byte aligned", who, t);
    SLIC_REQUIRE(!(d.flags & SLIC_MT_VEC) || (all & 15) == 0, "%s: tensor %d: flagged for float4 access but not 16-byte aligned", who, t);
    SLIC_REQUIRE((d.flags & ~(SLIC_MT_VEC | SLIC_MT_NESTEROV | SLIC_MT_FIRST)) == 0, "%s: tensor %d: unknown flags 0x%x", who, t, d.flags);
    for (int k = 0; k < SLIC_MT_HYPER; ++k) SLIC_REQUIRE(isfinite(d.h[k]), "%s: tensor %d: hyper-parameter %d is not finite", who, t, k);
    if (op == MT_ADAM) SLIC_REQUIRE(d.h[6] > 0.0, "%s: tensor %d: sqrt(bc2) must be positive (step >= 1, beta2 < 1)", who, t);
  }
  return SLIC_OK;
}

template <int OP>
static int mt_run(const char* who, const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int all_first,
                  void* stream) {
  SLIC_REQUIRE(map && desc && desc_host && n_items > 0 && n_tensors > 0, "%s: NULL table or nothing to do", who);
  SLIC_REQUIRE(((uintptr_t)map & 7) == 0 && ((uintptr_t)desc & 15) == 0, "%s: tables not aligned", who);
  const int rc = mt_validate(who, OP, desc_host, n_tensors);
  if (rc != SLIC_OK) return rc;
  int cus = slic_device_cus();
  if (cus <= 0) cus = 256;
  const int64_t cap = (int64_t)cus * MT_BLOCKS_PER_CU;
  const int grid = (int)(n_items < cap ? n_items : cap);
  mt_kernel<OP><<<dim3(grid), dim3(MT_THREADS), 0, S_(stream)>>>((const int2*)map, n_items, (const MtDesc*)desc, n_tensors, all_first);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_multi_tensor_chunk(void) { return MT_CHUNK; }

extern "C" int slic_multi_sgd(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int all_first, void* stream) {
  return mt_run<MT_SGD>("slic_multi_sgd", map, n_items, desc, desc_host, n_tensors, all_first ? 1 : 0, stream);
}

extern "C" int slic_multi_adam(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, void* stream) {
  return mt_run<MT_ADAM>("slic_multi_adam", map, n_items, desc, desc_host, n_tensors, 0, stream);
}

extern "C" int slic_multi_ema(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, void* stream) {
  return mt_run<MT_EMA>("slic_multi_ema", map, n_items, desc, desc_host, n_tensors, 0, stream);
}
