// Multi-tensor parameter updates (optim.py): SGD, Adam, LARS and the MoCo key-encoder EMA, each as ONE launch over every tensor of every
// parameter group of one optimizer.  A pure stream: momentum SGD and LARS read p, g, buf and write p, buf (five streams of 4 bytes per
// element), Adam reads p, g, m, v and writes p, m, v (seven), the EMA reads k, q and writes k (three).  Per-tensor norms over the same
// tables (LARS's trust ratios, gradient clipping, the logged gradient norm): second half of this comment.
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
//   LARS  h[0] lr, h[1] momentum, h[2] trust_coefficient, h[3] weight_decay; SLIC_MT_ADAPT, SLIC_MT_FIRST (or all_first)
//         u = g + wd p;  v = adapt ? q[t] u : u;  buf = first ? v : mom buf + v;  p -= lr buf;  mom == 0: p -= lr v
//         q[t] is read from device memory (the launch's `ratios`), where the fold below left it; a tensor without SLIC_MT_ADAPT never
//         reads it and is SGD's chain with dampening 0, bit for bit.
//
// Norms, two launches, both deterministic (no floating-point atomics; the same inputs give the same bits):
//   norm pass  mt_norm_kernel walks the map as the updates do (same skip rules, float4 / element paths, tail) and writes per item two
//              doubles, partials[item][2]:  LARS mode  {sum p^2, sum u^2} with u = wd != 0 ? fmaf(wd, p, g) : g in fp32, the value the
//              update will form;  gradient modes  {0, sum g^2}  or  {0, max |g|}.  Every fp32 element is widened to double, squares and
//              sums are double (fma).  A thread adds its elements in ascending order; the workgroup's 256 partial sums are folded in
//              a fixed order: the shuffle ladder (offsets 32 .. 1) inside a wave, then the four wave sums through LDS, wave 0 first.
//              A skipped item writes zeros, so the fold reads nothing that was not written.
//   fold       mt_fold_kernel: one wave per tensor.  The tensor's first item is the running sum of ceil(n / CHUNK) over desc[] (every wave
//              walks desc[].n; the host checks the sum against n_items).  Lane l adds items first + l, first + l + 64, ... in
//              ascending order, the same ladder folds the 64 lanes, lane 0 writes wnorm[t], unorm[t] (fp32, rounded once from the
//              double square root) and q[t] = (wnorm > 0 && unorm > 0) ? trust_coefficient wnorm / unorm : 1 (double, rounded once).
//              Gradient modes run as ONE workgroup, which keeps the tensors' double sums in LDS and adds them in tensor order into
//              total[0] = the norm over all tensors and total[1] = min(max_norm (1 / (total[0] + 1e-6)), 1) in fp32, the roundings of
//              torch.nn.utils.clip_grad_norm_ (a reciprocal, then a product); NaN stays NaN.  The max of the inf-norm carries NaN too.
//   scale      mt_scale_kernel: g *= total[1], read from device memory.  A workgroup that reads a coefficient >= 1 returns before
//              it touches a gradient (torch multiplies by exactly 1.0 there: the same bits); NaN is not >= 1 and takes the multiply.
#include <math.h>
#include <string.h>
#include "common.h"

#define MT_THREADS 256
#define MT_CHUNK 4096
#define MT_VPT (MT_CHUNK / 4 / MT_THREADS)      // float4 per thread per stream per item
#define MT_BLOCKS_PER_CU 8
#define MT_FOLD_THREADS 1024                    // 16 waves: 16 tensors in flight per workgroup of the fold
enum { MT_SGD = 0, MT_ADAM = 1, MT_EMA = 2, MT_LARS = 3, MT_GRAD = 4 };        // MT_GRAD: the gradient-only operations (norm, scale)

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
  bool wd, mom, nesterov, first, adapt;
};

template <int OP>
__device__ __forceinline__ MtHyper mt_hyper(const MtDesc& d, int all_first, const float* __restrict__ ratios, int t) {
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
  } else if constexpr (OP == MT_LARS) {
    h.a = (float)d.h[0]; h.b = (float)d.h[1]; h.d = (float)d.h[3];
    h.wd = d.h[3] != 0.0;
    h.mom = d.h[1] != 0.0;
    h.first = all_first || (d.flags & SLIC_MT_FIRST);
    h.adapt = d.flags & SLIC_MT_ADAPT;
    h.e = h.adapt ? ratios[t] : 1.f;                          // the trust ratio q[t]: only an adaptive tensor reads it
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
  } else if constexpr (OP == MT_LARS) {
    if (h.wd) g = fmaf(h.d, p, g);
    if (h.adapt) g = h.e * g;
    float u = g;
    if (h.mom) {
      s1 = h.first ? g : fmaf(h.b, s1, g);
      u = s1;
    }
    p = fmaf(-h.a, u, p);
  } else {
    p = fmaf(p, h.a, g * h.b);
  }
}

template <int OP>
__global__ __launch_bounds__(MT_THREADS) void mt_kernel(const int2* __restrict__ map, int n_items, const MtDesc* __restrict__ desc, int n_tensors,
                                                       int all_first, const float* __restrict__ ratios) {
  constexpr bool S1 = OP != MT_EMA, S2 = OP == MT_ADAM;
  constexpr bool SGDLIKE = OP == MT_SGD || OP == MT_LARS;     // a momentum buffer that may be absent, and is defined by a first step
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int2 it = map[item];
    if (it.x < 0 || it.x >= n_tensors || it.y < 0) continue;
    const MtDesc& d = desc[it.x];
    const int64_t off = (int64_t)it.y * MT_CHUNK;
    if (off >= d.n) continue;
    const int len = (int)(d.n - off < (int64_t)MT_CHUNK ? d.n - off : (int64_t)MT_CHUNK);
    const MtHyper h = mt_hyper<OP>(d, all_first, ratios, it.x);
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
          if (use1 && !(SGDLIKE && h.first)) A[k] = ((const gf32x4*)s1)[i];
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
      if (use1 && !(SGDLIKE && h.first)) aj = s1[i];
      if (S2) bj = s2[i];
      mt_update<OP>(h, pj, g[i], aj, bj);
      p[i] = pj;
      if (use1) s1[i] = aj;
      if (S2) s2[i] = bj;
    }
  }
}

// the item's tensor and its elements [off, off + len); false: the entry names no tensor or no chunk of its tensor (skipped, never followed)
__device__ __forceinline__ bool mt_item(const int2* __restrict__ map, int item, const MtDesc* __restrict__ desc, int n_tensors, int* t, int64_t* off,
                                        int* len) {
  const int2 it = map[item];
  if (it.x < 0 || it.x >= n_tensors || it.y < 0) return false;
  const int64_t n = desc[it.x].n;
  *t = it.x;
  *off = (int64_t)it.y * MT_CHUNK;
  if (*off >= n) return false;
  *len = (int)(n - *off < (int64_t)MT_CHUNK ? n - *off : (int64_t)MT_CHUNK);
  return true;
}

// the larger of two, NaN if either is
__device__ __forceinline__ double mt_max(double a, double b) { return (a != a || a > b) ? a : b; }

// the 64 lanes' values folded by the shuffle ladder, offsets 32 .. 1: lane 0 holds the result
template <bool MAX>
__device__ __forceinline__ double mt_wave_fold(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_down(v, o);
    v = MAX ? mt_max(v, u) : v + u;
  }
  return v;
}

template <int MODE>
__global__ __launch_bounds__(MT_THREADS) void mt_norm_kernel(const int2* __restrict__ map, int n_items, const MtDesc* __restrict__ desc, int n_tensors,
                                                            double* __restrict__ partials) {
  constexpr bool LARS = MODE == SLIC_MT_NORM_LARS, INF = MODE == SLIC_MT_NORM_GRAD_INF;
  constexpr int WAVES = MT_THREADS / 64;
  __shared__ double sh[2][WAVES][2];                           // two sets, used in turn: one barrier per item
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int turn = 0;
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    int t, len;
    int64_t off;
    if (!mt_item(map, item, desc, n_tensors, &t, &off, &len)) {
      if (threadIdx.x == 0) partials[2 * (int64_t)item] = 0.0, partials[2 * (int64_t)item + 1] = 0.0;
      continue;
    }
    const MtDesc& d = desc[t];
    const float wd = (float)d.h[3];
    const bool has_wd = LARS && d.h[3] != 0.0;
    const gfloat* p = LARS ? (const gfloat*)d.p + off : nullptr;
    const gfloat* g = (const gfloat*)d.g + off;
    double a0 = 0.0, a1 = 0.0;                                 // this thread's sums (max), its elements in ascending order
    auto add = [&](float pj, float gj) {
      if constexpr (LARS) {
        const float u = has_wd ? fmaf(wd, pj, gj) : gj;
        const double dp = (double)pj, du = (double)u;
        a0 = fma(dp, dp, a0);
        a1 = fma(du, du, a1);
      } else if constexpr (INF) {
        a1 = mt_max(fabs((double)gj), a1);
      } else {
        const double dg = (double)gj;
        a1 = fma(dg, dg, a1);
      }
    };
    int done = 0;
    if (d.flags & SLIC_MT_VEC) {
      const int nv = len >> 2;
      done = nv << 2;
      f32x4 P[MT_VPT] = {}, G[MT_VPT] = {};
#pragma unroll
      for (int k = 0; k < MT_VPT; ++k) {
        const int i = threadIdx.x + k * MT_THREADS;
        if (i < nv) {
          if (LARS) P[k] = ((const gf32x4*)p)[i];
          G[k] = ((const gf32x4*)g)[i];
        }
      }
#pragma unroll
      for (int k = 0; k < MT_VPT; ++k) {
        const int i = threadIdx.x + k * MT_THREADS;
        if (i < nv) {
#pragma unroll
          for (int j = 0; j < 4; ++j) add(P[k][j], G[k][j]);
        }
      }
    }
    for (int i = done + threadIdx.x; i < len; i += MT_THREADS) add(LARS ? p[i] : 0.f, g[i]);
    a0 = LARS ? mt_wave_fold<false>(a0) : 0.0;
    a1 = mt_wave_fold<INF>(a1);
    if (lane == 0) sh[turn][wave][0] = a0, sh[turn][wave][1] = a1;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s0 = sh[turn][0][0], s1 = sh[turn][0][1];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) {
        s0 += sh[turn][w][0];
        s1 = INF ? mt_max(s1, sh[turn][w][1]) : s1 + sh[turn][w][1];
      }
      partials[2 * (int64_t)item] = s0;
      partials[2 * (int64_t)item + 1] = s1;
    }
    turn ^= 1;      // the other set next: its last reader (thread 0, two items ago) has passed the barrier above since
  }
}

// norms [3][n_tensors]: wnorm, unorm, q.  total [2] (gradient modes, which run as one workgroup): the norm over all tensors, the clip coefficient.
template <int MODE>
__global__ __launch_bounds__(MT_FOLD_THREADS) void mt_fold_kernel(const MtDesc* __restrict__ desc, int n_tensors, int n_items,
                                                                 const double* __restrict__ partials, float max_norm, float* __restrict__ norms,
                                                                 float* __restrict__ total) {
  constexpr bool GRAD = MODE != SLIC_MT_NORM_LARS, INF = MODE == SLIC_MT_NORM_GRAD_INF;
  constexpr int WAVES = MT_FOLD_THREADS / 64;
  __shared__ double sums[MT_FOLD_THREADS];                     // gradient modes: the double sums of up to MT_FOLD_THREADS tensors
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * WAVES;
  int64_t first = 0;                                           // tensor t's first item: the items of the tensors before it
  double tot = 0.0;                                            // thread 0
  for (int base = 0; base < n_tensors; base += MT_FOLD_THREADS) {
    const int cnt = n_tensors - base < MT_FOLD_THREADS ? n_tensors - base : MT_FOLD_THREADS;
    for (int j = 0; j < cnt; ++j) {
      const int t = base + j;
      const int64_t n = desc[t].n;
      const int64_t nch = n > 0 ? (n + (MT_CHUNK - 1)) / MT_CHUNK : 0;
      if (t % n_waves == wave) {
        const int64_t end = first + nch <= (int64_t)n_items ? first + nch : first;      // a table that disagrees with n_items: nothing is read
        double a0 = 0.0, a1 = 0.0;
        for (int64_t i = first + lane; i < end; i += 64) {
          a0 += partials[2 * i];
          a1 = INF ? mt_max(a1, partials[2 * i + 1]) : a1 + partials[2 * i + 1];
        }
        a0 = mt_wave_fold<false>(a0);
        a1 = mt_wave_fold<INF>(a1);
        if (lane == 0) {
          const double wn = sqrt(a0), un = INF ? a1 : sqrt(a1);
          norms[t] = (float)wn;
          norms[n_tensors + t] = (float)un;
          norms[2 * (int64_t)n_tensors + t] = (!GRAD && wn > 0.0 && un > 0.0) ? (float)(desc[t].h[2] * wn / un) : 1.f;
          if (GRAD) sums[j] = a1;
        }
      }
      first += nch;
    }
    if (GRAD) {
      __syncthreads();
      if (threadIdx.x == 0)
        for (int j = 0; j < cnt; ++j) tot = INF ? mt_max(tot, sums[j]) : tot + sums[j];      // in tensor order
      __syncthreads();
    }
  }
  if (GRAD && threadIdx.x == 0) {
    const float tn = (float)(INF ? tot : sqrt(tot));
    const float coef = (1.f / (tn + 1e-6f)) * max_norm;        // torch: max_norm / tensor is tensor.reciprocal() * max_norm
    total[0] = tn;
    total[1] = coef > 1.f ? 1.f : coef;                        // NaN stays NaN
  }
}

__global__ __launch_bounds__(MT_THREADS) void mt_scale_kernel(const int2* __restrict__ map, int n_items, const MtDesc* __restrict__ desc, int n_tensors,
                                                             const float* __restrict__ total) {
  const float c = total[1];
  if (c >= 1.f) return;                                        // nothing clips: no gradient is touched.  NaN goes on
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    int t, len;
    int64_t off;
    if (!mt_item(map, item, desc, n_tensors, &t, &off, &len)) continue;
    const MtDesc& d = desc[t];
    gfloat* g = (gfloat*)d.g + off;
    int done = 0;
    if (d.flags & SLIC_MT_VEC) {
      const int nv = len >> 2;
      done = nv << 2;
      f32x4 G[MT_VPT];
#pragma unroll
      for (int k = 0; k < MT_VPT; ++k) {
        const int i = threadIdx.x + k * MT_THREADS;
        if (i < nv) G[k] = ((const gf32x4*)g)[i];
      }
#pragma unroll
      for (int k = 0; k < MT_VPT; ++k) {
        const int i = threadIdx.x + k * MT_THREADS;
        if (i < nv) {
          f32x4 q = G[k];
#pragma unroll
          for (int j = 0; j < 4; ++j) q[j] = q[j] * c;
          ((gf32x4*)g)[i] = q;
        }
      }
    }
    for (int i = done + threadIdx.x; i < len; i += MT_THREADS) g[i] = g[i] * c;
  }
}

// every descriptor names memory the kernel may touch as it will touch it: fp32-aligned pointers, the state the operation needs, a
// vector flag only over 16-byte aligned pointers, finite hyper-parameters, no flag the operation does not know.
// items (optional): the work items the tensors make, sum of ceil(n / CHUNK); adaptive (optional): whether a tensor carries SLIC_MT_ADAPT
static int mt_validate(const char* who, int op, const void* desc_host, int n_tensors, int64_t* items = nullptr, bool* adaptive = nullptr) {
  const int known = op == MT_SGD    ? SLIC_MT_VEC | SLIC_MT_NESTEROV | SLIC_MT_FIRST
                    : op == MT_LARS ? SLIC_MT_VEC | SLIC_MT_FIRST | SLIC_MT_ADAPT
                    : op == MT_GRAD ? SLIC_MT_VEC
                                    : SLIC_MT_VEC | SLIC_MT_NESTEROV | SLIC_MT_FIRST;      // Adam, EMA: as they always were
  int64_t sum = 0;
  bool any = false;
  for (int t = 0; t < n_tensors; ++t) {
    MtDesc d;
    memcpy(&d, (const char*)desc_host + (size_t)t * sizeof(MtDesc), sizeof(MtDesc));
    SLIC_REQUIRE(d.n > 0 && d.n <= (int64_t)INT32_MAX * MT_CHUNK, "%s: tensor %d: length %lld", who, t, (long long)d.n);
    const bool needp = op != MT_GRAD;
    SLIC_REQUIRE((!needp || d.p) && d.g, "%s: tensor %d: NULL parameter or gradient", who, t);
    const bool need1 = op == MT_ADAM || ((op == MT_SGD || op == MT_LARS) && d.h[1] != 0.0), need2 = op == MT_ADAM;
    SLIC_REQUIRE(!need1 || d.s1, "%s: tensor %d: NULL %s", who, t, op == MT_ADAM ? "exp_avg" : "momentum_buffer");
    SLIC_REQUIRE(!need2 || d.s2, "%s: tensor %d: NULL exp_avg_sq", who, t);
    const uint64_t all = (needp ? d.p : 0) | d.g | (need1 ? d.s1 : 0) | (need2 ? d.s2 : 0);
    SLIC_REQUIRE((all & 3) == 0, "%s: tensor %d: a pointer is not 4-byte aligned", who, t);
    SLIC_REQUIRE(!(d.flags & SLIC_MT_VEC) || (all & 15) == 0, "%s: tensor %d: flagged for float4 access but not 16-byte aligned", who, t);
    SLIC_REQUIRE((d.flags & ~known) == 0, "%s: tensor %d: unknown flags 0x%x", who, t, d.flags);
    for (int k = 0; k < SLIC_MT_HYPER; ++k) SLIC_REQUIRE(isfinite(d.h[k]), "%s: tensor %d: hyper-parameter %d is not finite", who, t, k);
    if (op == MT_ADAM) SLIC_REQUIRE(d.h[6] > 0.0, "%s: tensor %d: sqrt(bc2) must be positive (step >= 1, beta2 < 1)", who, t);
    if (op == MT_LARS) SLIC_REQUIRE(d.h[2] > 0.0, "%s: tensor %d: trust_coefficient must be positive", who, t);
    sum += (d.n + (MT_CHUNK - 1)) / MT_CHUNK;
    any = any || (d.flags & SLIC_MT_ADAPT);
  }
  if (items) *items = sum;
  if (adaptive) *adaptive = any;
  return SLIC_OK;
}

static int mt_grid(int n_items) {
  int cus = slic_device_cus();
  if (cus <= 0) cus = 256;
  const int64_t cap = (int64_t)cus * MT_BLOCKS_PER_CU;
  return (int)(n_items < cap ? n_items : cap);
}

static int mt_tables(const char* who, const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors) {
  SLIC_REQUIRE(map && desc && desc_host && n_items > 0 && n_tensors > 0, "%s: NULL table or nothing to do", who);
  SLIC_REQUIRE(((uintptr_t)map & 7) == 0 && ((uintptr_t)desc & 15) == 0, "%s: tables not aligned", who);
  return SLIC_OK;
}

static int mt_scratch(const char* who, const char* what, const void* ptr) {
  SLIC_REQUIRE(ptr && ((uintptr_t)ptr & 7) == 0, "%s: %s is NULL or not 8-byte aligned", who, what);
  return SLIC_OK;
}

template <int OP>
static int mt_run(const char* who, const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int all_first,
                  const float* ratios, void* stream) {
  int rc = mt_tables(who, map, n_items, desc, desc_host, n_tensors);
  if (rc != SLIC_OK) return rc;
  bool adaptive = false;
  rc = mt_validate(who, OP, desc_host, n_tensors, nullptr, &adaptive);
  if (rc != SLIC_OK) return rc;
  if (adaptive && (rc = mt_scratch(who, "ratios (a tensor carries SLIC_MT_ADAPT)", ratios)) != SLIC_OK) return rc;
  mt_kernel<OP><<<dim3(mt_grid(n_items)), dim3(MT_THREADS), 0, S_(stream)>>>((const int2*)map, n_items, (const MtDesc*)desc, n_tensors, all_first,
                                                                            ratios);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_multi_tensor_chunk(void) { return MT_CHUNK; }

extern "C" int slic_multi_sgd(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int all_first, void* stream) {
  return mt_run<MT_SGD>("slic_multi_sgd", map, n_items, desc, desc_host, n_tensors, all_first ? 1 : 0, nullptr, stream);
}

extern "C" int slic_multi_adam(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, void* stream) {
  return mt_run<MT_ADAM>("slic_multi_adam", map, n_items, desc, desc_host, n_tensors, 0, nullptr, stream);
}

extern "C" int slic_multi_ema(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, void* stream) {
  return mt_run<MT_EMA>("slic_multi_ema", map, n_items, desc, desc_host, n_tensors, 0, nullptr, stream);
}

extern "C" int slic_multi_lars(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int all_first,
                               const float* ratios, void* stream) {
  return mt_run<MT_LARS>("slic_multi_lars", map, n_items, desc, desc_host, n_tensors, all_first ? 1 : 0, ratios, stream);
}

static int mt_mode(const char* who, int mode) {
  SLIC_REQUIRE(mode == SLIC_MT_NORM_LARS || mode == SLIC_MT_NORM_GRAD_L2 || mode == SLIC_MT_NORM_GRAD_INF, "%s: unknown mode %d", who, mode);
  return SLIC_OK;
}

extern "C" int slic_multi_sqnorm(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, int mode,
                                 double* partials, void* stream) {
  const char* who = "slic_multi_sqnorm";
  int rc = mt_tables(who, map, n_items, desc, desc_host, n_tensors);
  if (rc == SLIC_OK) rc = mt_mode(who, mode);
  if (rc == SLIC_OK) rc = mt_scratch(who, "partials", partials);
  if (rc == SLIC_OK) rc = mt_validate(who, mode == SLIC_MT_NORM_LARS ? MT_LARS : MT_GRAD, desc_host, n_tensors);
  if (rc != SLIC_OK) return rc;
  const dim3 grid(mt_grid(n_items)), block(MT_THREADS);
  const int2* m = (const int2*)map;
  const MtDesc* d = (const MtDesc*)desc;
  if (mode == SLIC_MT_NORM_LARS) mt_norm_kernel<SLIC_MT_NORM_LARS><<<grid, block, 0, S_(stream)>>>(m, n_items, d, n_tensors, partials);
  else if (mode == SLIC_MT_NORM_GRAD_L2) mt_norm_kernel<SLIC_MT_NORM_GRAD_L2><<<grid, block, 0, S_(stream)>>>(m, n_items, d, n_tensors, partials);
  else mt_norm_kernel<SLIC_MT_NORM_GRAD_INF><<<grid, block, 0, S_(stream)>>>(m, n_items, d, n_tensors, partials);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_multi_norm_fold(const void* desc, const void* desc_host, int n_tensors, int n_items, const double* partials, int mode,
                                    double max_norm, float* norms, float* total, void* stream) {
  const char* who = "slic_multi_norm_fold";
  SLIC_REQUIRE(desc && desc_host && n_items > 0 && n_tensors > 0, "%s: NULL table or nothing to do", who);
  SLIC_REQUIRE(((uintptr_t)desc & 15) == 0, "%s: tables not aligned", who);
  int rc = mt_mode(who, mode);
  if (rc == SLIC_OK) rc = mt_scratch(who, "partials", partials);
  if (rc == SLIC_OK) rc = mt_scratch(who, "norms", norms);
  const bool grad = mode != SLIC_MT_NORM_LARS;
  if (rc == SLIC_OK && grad) rc = mt_scratch(who, "total", total);
  if (rc != SLIC_OK) return rc;
  SLIC_REQUIRE(isfinite(max_norm), "%s: max_norm is not finite", who);
  int64_t items = 0;
  rc = mt_validate(who, grad ? MT_GRAD : MT_LARS, desc_host, n_tensors, &items);
  if (rc != SLIC_OK) return rc;
  SLIC_REQUIRE(items == (int64_t)n_items, "%s: the tensors make %lld work items, not %d", who, (long long)items, n_items);
  const MtDesc* d = (const MtDesc*)desc;
  const dim3 block(MT_FOLD_THREADS);
  const int waves = MT_FOLD_THREADS / 64;
  if (mode == SLIC_MT_NORM_LARS) {
    int blocks = (n_tensors + waves - 1) / waves;
    if (blocks > 64) blocks = 64;
    mt_fold_kernel<SLIC_MT_NORM_LARS><<<dim3(blocks), block, 0, S_(stream)>>>(d, n_tensors, n_items, partials, 0.f, norms, total);
  } else if (mode == SLIC_MT_NORM_GRAD_L2) {
    mt_fold_kernel<SLIC_MT_NORM_GRAD_L2><<<dim3(1), block, 0, S_(stream)>>>(d, n_tensors, n_items, partials, (float)max_norm, norms, total);
  } else {
    mt_fold_kernel<SLIC_MT_NORM_GRAD_INF><<<dim3(1), block, 0, S_(stream)>>>(d, n_tensors, n_items, partials, (float)max_norm, norms, total);
  }
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_multi_scale(const void* map, int n_items, const void* desc, const void* desc_host, int n_tensors, const float* total,
                                void* stream) {
  const char* who = "slic_multi_scale";
  int rc = mt_tables(who, map, n_items, desc, desc_host, n_tensors);
  if (rc == SLIC_OK) rc = mt_scratch(who, "total", total);
  if (rc == SLIC_OK) rc = mt_validate(who, MT_GRAD, desc_host, n_tensors);
  if (rc != SLIC_OK) return rc;
  mt_scale_kernel<<<dim3(mt_grid(n_items)), dim3(MT_THREADS), 0, S_(stream)>>>((const int2*)map, n_items, (const MtDesc*)desc, n_tensors, total);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
