// Clip transforms (coclr_utils/transforms.py): a chain of tensor augmentations on a batch of clips as ONE gather kernel.
//   input   uint8 [N, H, W, 3] (with or without the /255 of ToFloatTensorInZeroOne) or fp32 [3, N, H, W], one per clip
//   output  fp32 [B, 3, N, Ho, Wo] contiguous
// The host planner (coclr_utils/transforms.py) folds a chain into a per-clip record:
//   geometry  out pixel (y, x) --map b--> (ry, rx) --[bilinear resample: four taps]--> map a --> source pixel | fill
//   colour    up to SLIC_CLIPTF_MAX_OPS of brightness / contrast / saturation / gray, each with a per-frame factor array [N]
//   normalise (x - mean) / std per channel
// This file is compiled with -ffp-contract=off (FLAGS_cliptf): every a * b + c below rounds twice, as the separate torch ops of the
// reference do, so everything except the contrast mean and the bilinear weights reproduces the reference bit for bit.
//
// Table (one device buffer, filled from one pinned host buffer per call; the host copy is what the entry points validate):
//   floats [0, 8)                 mean[3], std[3], 0, 0
//   bytes  [32, 32 + B * 144)     B records `CtClip`:
//        u64 src, src_bytes       device address and byte size of the clip
//        i32 Hs, Ws               source frame size
//        i32 flags                bit 0: resample, bit 1: uint8 taps may be read as packed pairs (map a covers its image, Wa >= 2)
//        i32 Ha, Wa               size of the image the resample reads (map a's domain)
//        f32 sc_y, sc_x           source step per output pixel (F.interpolate's: 1 / scale_factor, or in / out for a size)
//        i32 nops
//        map a, map b             8 x 4 bytes each: i32 y0, y1, x0, x1 (the rectangle that maps to data; outside it: fill),
//                                 i32 dy, dx, mx (target y = y + dy, target x = mx * x + dx, mx = +-1), f32 fill
//                                 without a resample only map b is used and its target is the source
//        i32 op_kind[4]           SLIC_CLIPTF_BRIGHTNESS ...
//        i32 op_fac[4]            index (in floats, from the table's start) of the op's factor array [N]
//   floats after the records      the factor arrays
//
// Launch: grid (row bands, N, B), 256 threads; a thread makes four consecutive pixels of a row (12 floats) at a time, grouped so that
// the stores of channel 0 are 16-byte aligned; rows whose start is not aligned get a scalar head and tail.
// Contrast needs the mean gray of the whole frame as it is BEFORE the contrast op: the stats launch (same grid, same partition)
// evaluates geometry + the preceding colour ops, reduces gray per (clip, frame, band) in a fixed tree (thread order, xor shuffles,
// four wave sums in order) and writes one partial per block; apply adds the bands in ascending order.  No atomics, no waiting
// between workgroups: the same input gives the same bits.
#include <math.h>
#include <string.h>
#include "common.h"

#define CT_THREADS 256
#define CT_HEAD_FLOATS 8
#define CT_MAX_BANDS 64

struct CtMap {
  int y0, y1, x0, x1, dy, dx, mx;
  float fill;
};
struct CtClip {
  uint64_t src, src_bytes;
  int Hs, Ws, flags, Ha, Wa;
  float sc_y, sc_x;
  int nops;
  CtMap a, b;
  int op_kind[SLIC_CLIPTF_MAX_OPS], op_fac[SLIC_CLIPTF_MAX_OPS];
};
static_assert(sizeof(CtClip) == SLIC_CLIPTF_REC_BYTES, "record layout is part of the ABI");

struct __attribute__((packed, aligned(4))) CtW3 { uint32_t w[3]; };
struct __attribute__((packed, aligned(4))) CtW4 { uint32_t w[4]; };

// rows per band: about one 4-pixel item per thread, at most CT_MAX_BANDS bands per frame
static inline int ct_band_rows(int Ho, int Wo) {
  const int G = (Wo + 6) / 4;
  int br = CT_THREADS / G;
  const int cap = (int)slic_cdiv(Ho, CT_MAX_BANDS);
  if (br < cap) br = cap;
  return br < 1 ? 1 : br;
}

__device__ __forceinline__ bool ct_in(const CtMap& m, int y, int x) { return y >= m.y0 && y < m.y1 && x >= m.x0 && x < m.x1; }
// a byte as a float; lut (the /255 kind): the 256 quotients b / 255.f, divided once per workgroup instead of once per tap
__device__ __forceinline__ float ct_u8(uint32_t v, const float* lut) { return lut ? lut[v & 0xffu] : (float)(v & 0xffu); }
__device__ __forceinline__ float ct_gray(float r, float g, float b) { return 0.2989f * r + 0.5870f * g + 0.1140f * b; }
__device__ __forceinline__ float ct_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// one source pixel, (sy, sx) inside the frame
template <int KIND>
__device__ __forceinline__ void ct_src(const CtClip& c, const float* lut, int N, int n, int sy, int sx, float px[3]) {
  const size_t idx = ((size_t)n * c.Hs + sy) * c.Ws + sx;
  if constexpr (KIND == SLIC_CLIPTF_SRC_F32) {
    const float* p = (const float*)c.src;
    const size_t plane = (size_t)N * c.Hs * c.Ws;
    px[0] = p[idx];
    px[1] = p[plane + idx];
    px[2] = p[2 * plane + idx];
  } else {
    const uint8_t* p = (const uint8_t*)c.src + idx * 3;
    px[0] = ct_u8(p[0], lut);
    px[1] = ct_u8(p[1], lut);
    px[2] = ct_u8(p[2], lut);
  }
}

// pixel (y, x) of the image that map m shows of the source
template <int KIND>
__device__ __forceinline__ void ct_fetch(const CtClip& c, const CtMap& m, const float* lut, int N, int n, int y, int x, float px[3]) {
  if (ct_in(m, y, x)) {
    ct_src<KIND>(c, lut, N, n, y + m.dy, m.mx * x + m.dx, px);
  } else {
    px[0] = px[1] = px[2] = m.fill;
  }
}

struct CtTap {
  int i0, i1;
  float l0, l1;      // weights of i0 and i1
};
// F.interpolate(mode='bilinear', align_corners=False): source index of output index o
__device__ __forceinline__ CtTap ct_tap(float scale, int o, int size) {
  float f = scale * ((float)o + 0.5f) - 0.5f;
  if (f < 0.f) f = 0.f;
  int i0 = (int)fminf(f, 1.0e9f);
  const float l1 = f - (float)i0;
  if (i0 > size - 1) i0 = size - 1;
  CtTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < size - 1 ? 1 : 0);
  t.l1 = l1;
  t.l0 = 1.f - l1;
  return t;
}

// two adjacent uint8 pixels (6 bytes at p) as (bytes 0-3, bytes 4-5); [lo4, end4): the whole words inside the clip
__device__ __forceinline__ void ct_ld6(const uint8_t* p, uintptr_t lo4, uintptr_t end4, uint32_t& lo, uint32_t& hi) {
  const uintptr_t a = (uintptr_t)p & ~(uintptr_t)3;
  const unsigned sh = ((unsigned)(uintptr_t)p & 3u) * 8u;
  if (a >= lo4 && a + 12 <= end4) {
    const CtW3 w = *(const CtW3*)a;
    lo = __funnelshift_r(w.w[0], w.w[1], sh);
    hi = __funnelshift_r(w.w[1], w.w[2], sh);
  } else {
    lo = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    hi = (uint32_t)p[4] | ((uint32_t)p[5] << 8);
  }
}

// the pixel at (ry, rx) of the resampled image
template <int KIND>
__device__ __forceinline__ void ct_bilinear(const CtClip& c, const float* lut, int N, int n, int ry, int rx, uintptr_t lo4, uintptr_t end4, float px[3]) {
  const CtTap ty = ct_tap(c.sc_y, ry, c.Ha), tx = ct_tap(c.sc_x, rx, c.Wa);
  float v[2][2][3];
  if (KIND != SLIC_CLIPTF_SRC_F32 && (c.flags & 2)) {
    // both taps of a row are adjacent in memory: read the pair xa, xa + 1 as packed words
    const int xa = min(tx.i0, c.Wa - 2);
    const int sA = c.a.mx * xa + c.a.dx, sB = sA + c.a.mx;
    const int s0 = min(sA, sB);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int sy = (r ? ty.i1 : ty.i0) + c.a.dy;
      uint32_t lo, hi;
      ct_ld6((const uint8_t*)c.src + (((size_t)n * c.Hs + sy) * c.Ws + s0) * 3, lo4, end4, lo, hi);
      float P[2][3];
      P[0][0] = ct_u8(lo, lut);
      P[0][1] = ct_u8(lo >> 8, lut);
      P[0][2] = ct_u8(lo >> 16, lut);
      P[1][0] = ct_u8(lo >> 24, lut);
      P[1][1] = ct_u8(hi, lut);
      P[1][2] = ct_u8(hi >> 8, lut);
      const int ia = c.a.mx > 0 ? 0 : 1;       // which of the two holds image pixel xa
      const int k0 = tx.i0 == xa ? ia : 1 - ia, k1 = tx.i1 == xa ? ia : 1 - ia;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        v[r][0][ch] = P[k0][ch];
        v[r][1][ch] = P[k1][ch];
      }
    }
  } else {
    ct_fetch<KIND>(c, c.a, lut, N, n, ty.i0, tx.i0, v[0][0]);
    ct_fetch<KIND>(c, c.a, lut, N, n, ty.i0, tx.i1, v[0][1]);
    ct_fetch<KIND>(c, c.a, lut, N, n, ty.i1, tx.i0, v[1][0]);
    ct_fetch<KIND>(c, c.a, lut, N, n, ty.i1, tx.i1, v[1][1]);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    px[ch] = ty.l0 * (tx.l0 * v[0][0][ch] + tx.l1 * v[0][1][ch]) + ty.l1 * (tx.l0 * v[1][0][ch] + tx.l1 * v[1][1][ch]);
}

// output pixels x in [xs, xs + 4) ∩ [xlo, xhi) of row y, after the geometry: v[ch][x - xs]
template <int KIND>
__device__ __forceinline__ void ct_gather(const CtClip& c, const float* lut, int N, int n, int y, int xs, int xlo, int xhi, uintptr_t lo4, uintptr_t end4, float v[3][4]) {
  const bool resample = c.flags & 1;
  const bool inside = xhi - xlo == 4 && y >= c.b.y0 && y < c.b.y1 && xlo >= c.b.x0 && xhi <= c.b.x1;
  if (inside && !resample) {
    // four source pixels in a row, ascending or descending
    const int sy = y + c.b.dy;
    const int sa = c.b.mx * xlo + c.b.dx, sb = c.b.mx * (xhi - 1) + c.b.dx;
    const int s0 = min(sa, sb);
    const size_t idx = ((size_t)n * c.Hs + sy) * c.Ws + s0;
    float t[3][4];
    if constexpr (KIND == SLIC_CLIPTF_SRC_F32) {
      const size_t plane = (size_t)N * c.Hs * c.Ws;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float* p = (const float*)c.src + ch * plane + idx;
        if (((uintptr_t)p & 15) == 0) {
          const f32x4 q = *(const f32x4*)p;
          t[ch][0] = q[0]; t[ch][1] = q[1]; t[ch][2] = q[2]; t[ch][3] = q[3];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) t[ch][j] = p[j];
        }
      }
    } else {
      const uint8_t* p = (const uint8_t*)c.src + idx * 3;
      const uintptr_t a = (uintptr_t)p & ~(uintptr_t)3;
      uint32_t q[3];
      if (a >= lo4 && a + 16 <= end4) {
        const unsigned sh = ((unsigned)(uintptr_t)p & 3u) * 8u;
        const CtW4 w = *(const CtW4*)a;
        q[0] = __funnelshift_r(w.w[0], w.w[1], sh);
        q[1] = __funnelshift_r(w.w[1], w.w[2], sh);
        q[2] = __funnelshift_r(w.w[2], w.w[3], sh);
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          q[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int k = 3 * j + ch;
          t[ch][j] = ct_u8(q[k >> 2] >> (8 * (k & 3)), lut);
        }
    }
    const bool rev = c.b.mx < 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int j = 0; j < 4; ++j) v[ch][j] = rev ? t[ch][3 - j] : t[ch][j];
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = xs + j;
    float px[3] = {0.f, 0.f, 0.f};
    if (x >= xlo && x < xhi) {
      if (!ct_in(c.b, y, x)) {
        px[0] = px[1] = px[2] = c.b.fill;
      } else if (resample) {
        ct_bilinear<KIND>(c, lut, N, n, y + c.b.dy, c.b.mx * x + c.b.dx, lo4, end4, px);
      } else {
        ct_src<KIND>(c, lut, N, n, y + c.b.dy, c.b.mx * x + c.b.dx, px);
      }
    }
    v[0][j] = px[0]; v[1][j] = px[1]; v[2][j] = px[2];
  }
}

// colour op `kind` with the frame's factor f on four pixels (mean: the frame's mean gray, contrast only)
__device__ __forceinline__ void ct_colour(int kind, float f, float mean, float v[3][4]) {
  const float g1 = 1.f - f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float r = v[0][j], g = v[1][j], b = v[2][j];
    if (kind == SLIC_CLIPTF_GRAY) {
      const float gr = ct_gray(r, g, b);
      v[0][j] = gr * f + r * g1;
      v[1][j] = gr * f + g * g1;
      v[2][j] = gr * f + b * g1;
    } else {
      const float o = kind == SLIC_CLIPTF_BRIGHTNESS ? 0.f : kind == SLIC_CLIPTF_CONTRAST ? mean : ct_gray(r, g, b);
      v[0][j] = ct_clamp01(f * r + g1 * o);
      v[1][j] = ct_clamp01(f * g + g1 * o);
      v[2][j] = ct_clamp01(f * b + g1 * o);
    }
  }
}

template <int KIND, bool STATS>
__global__ __launch_bounds__(CT_THREADS) void cliptf_kernel(const char* __restrict__ table, int N, int Ho, int Wo, int normalize, int band_rows,
                                                           int nbands, float* __restrict__ ws, float* __restrict__ out) {
  __shared__ float wsum[CT_THREADS / 64];
  const int band = blockIdx.x, n = blockIdx.y, clip = blockIdx.z;
  const float* tf = (const float*)table;
  const CtClip& c = *(const CtClip*)(table + CT_HEAD_FLOATS * 4 + (size_t)clip * sizeof(CtClip));
  int ic = -1;                                   // position of the contrast op
  for (int k = 0; k < c.nops; ++k)
    if (c.op_kind[k] == SLIC_CLIPTF_CONTRAST) ic = k;
  if (STATS && ic < 0) return;
  __shared__ float lut255[256];
  static_assert(CT_THREADS == 256, "one quotient per thread");
  const float* lut = nullptr;
  if constexpr (KIND == SLIC_CLIPTF_SRC_U8_255) {
    lut255[threadIdx.x] = (float)threadIdx.x / 255.f;
    __syncthreads();
    lut = lut255;
  }
  const int nfirst = STATS ? ic : c.nops;
  float fac[SLIC_CLIPTF_MAX_OPS];
#pragma unroll
  for (int k = 0; k < SLIC_CLIPTF_MAX_OPS; ++k) fac[k] = k < c.nops ? tf[c.op_fac[k] + n] : 0.f;
  float mean = 0.f;
  if (!STATS && ic >= 0) {
    const float* part = ws + ((size_t)clip * N + n) * nbands;
    float s = 0.f;
    for (int k = 0; k < nbands; ++k) s += part[k];
    mean = s / (float)((int64_t)Ho * Wo);
  }
  float mu[3] = {0.f, 0.f, 0.f}, sd[3] = {1.f, 1.f, 1.f};
  if (!STATS && normalize) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      mu[ch] = tf[ch];
      sd[ch] = tf[3 + ch];
    }
  }
  const uintptr_t lo4 = (uintptr_t)(c.src + 3) & ~(uintptr_t)3, end4 = (uintptr_t)(c.src + c.src_bytes) & ~(uintptr_t)3;
  const int yb = band * band_rows;
  const int rows = min(band_rows, Ho - yb);
  const int G = (Wo & 3) ? (Wo + 6) / 4 : Wo / 4;
  const size_t plane = (size_t)N * Ho * Wo;
  float acc = 0.f;
  for (int it = threadIdx.x; it < rows * G; it += CT_THREADS) {
    const int rr = it / G, g = it - rr * G;
    const int y = yb + rr;
    const size_t e0 = (((size_t)clip * 3 * N + n) * Ho + y) * Wo;
    const int xs = 4 * g - (int)(e0 & 3);
    const int xlo = max(xs, 0), xhi = min(xs + 4, Wo);
    if (xlo >= xhi) continue;
    float v[3][4];
    ct_gather<KIND>(c, lut, N, n, y, xs, xlo, xhi, lo4, end4, v);
#pragma unroll
    for (int k = 0; k < SLIC_CLIPTF_MAX_OPS; ++k)
      if (k < nfirst) ct_colour(c.op_kind[k], fac[k], mean, v);
    if constexpr (STATS) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xs + j >= xlo && xs + j < xhi) acc += ct_gray(v[0][j], v[1][j], v[2][j]);
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (normalize) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[ch][j] = (v[ch][j] - mu[ch]) / sd[ch];
        }
        float* o = out + e0 + ch * plane + xs;
        if (xhi - xlo == 4 && ((uintptr_t)o & 15) == 0) {
          f32x4 q;
          q[0] = v[ch][0]; q[1] = v[ch][1]; q[2] = v[ch][2]; q[3] = v[ch][3];
          *(f32x4*)o = q;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (xs + j >= xlo && xs + j < xhi) o[j] = v[ch][j];
        }
      }
    }
  }
  if constexpr (STATS) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = wsum[0];
      for (int w = 1; w < CT_THREADS / 64; ++w) s += wsum[w];
      ws[((size_t)clip * N + n) * nbands + band] = s;
    }
  }
}

// a map whose rectangle lies in [0, H) x [0, W) and whose targets lie in [0, Ht) x [0, Wt)
static bool ct_map_ok(const CtMap& m, int H, int W, int Ht, int Wt) {
  if (!(0 <= m.y0 && m.y0 <= m.y1 && m.y1 <= H && 0 <= m.x0 && m.x0 <= m.x1 && m.x1 <= W)) return false;
  if (m.mx != 1 && m.mx != -1) return false;
  if (m.y0 == m.y1 || m.x0 == m.x1) return true;
  const int64_t ya = (int64_t)m.y0 + m.dy, yb = (int64_t)m.y1 - 1 + m.dy;
  const int64_t xa = (int64_t)m.mx * m.x0 + m.dx, xb = (int64_t)m.mx * (m.x1 - 1) + m.dx;
  return ya >= 0 && yb < Ht && xa >= 0 && xa < Wt && xb >= 0 && xb < Wt;
}

// every index a record can produce stays inside its clip and inside the table; *any_contrast: some clip has a contrast op
static int ct_validate(const char* who, const void* table_host, size_t table_bytes, int B, int N, int Ho, int Wo, int kind, int* any_contrast) {
  SLIC_REQUIRE(table_host && B > 0 && B <= 65535 && N > 0 && N <= 65535 && Ho > 0 && Wo > 0, "%s: bad args (1 <= B, N <= 65535, Ho, Wo > 0)", who);
  SLIC_REQUIRE(kind == SLIC_CLIPTF_SRC_U8 || kind == SLIC_CLIPTF_SRC_U8_255 || kind == SLIC_CLIPTF_SRC_F32, "%s: unknown input kind %d", who, kind);
  SLIC_REQUIRE((int64_t)Ho * Wo < ((int64_t)1 << 31), "%s: frame too large", who);
  const size_t first_fac = CT_HEAD_FLOATS + (size_t)B * sizeof(CtClip) / 4;
  SLIC_REQUIRE(table_bytes % 4 == 0 && table_bytes >= first_fac * 4, "%s: table shorter than its %d records", who, B);
  const size_t nfloat = table_bytes / 4;
  const size_t esz = kind == SLIC_CLIPTF_SRC_F32 ? 4 : 1;
  *any_contrast = 0;
  for (int i = 0; i < B; ++i) {
    CtClip c;
    memcpy(&c, (const char*)table_host + CT_HEAD_FLOATS * 4 + (size_t)i * sizeof(CtClip), sizeof(CtClip));
    SLIC_REQUIRE(c.src && c.Hs > 0 && c.Ws > 0 && (int64_t)c.Hs * c.Ws < ((int64_t)1 << 31), "%s: clip %d: bad source", who, i);
    SLIC_REQUIRE(c.src_bytes >= esz * 3 * (uint64_t)N * c.Hs * c.Ws, "%s: clip %d: source smaller than [N, Hs, Ws, 3]", who, i);
    SLIC_REQUIRE(esz == 1 || c.src % 4 == 0, "%s: clip %d: fp32 source not aligned", who, i);
    SLIC_REQUIRE(ct_map_ok(c.b, Ho, Wo, (c.flags & 1) ? (1 << 30) : c.Hs, (c.flags & 1) ? (1 << 30) : c.Ws), "%s: clip %d: map b leaves its target", who, i);
    if (c.flags & 1) {
      SLIC_REQUIRE(c.Ha > 0 && c.Wa > 0 && c.sc_y > 0.f && c.sc_x > 0.f && c.sc_y < 1e6f && c.sc_x < 1e6f, "%s: clip %d: bad resample", who, i);
      SLIC_REQUIRE(ct_map_ok(c.a, c.Ha, c.Wa, c.Hs, c.Ws), "%s: clip %d: map a leaves the source", who, i);
      if (c.flags & 2)
        SLIC_REQUIRE(c.Wa >= 2 && c.a.y0 == 0 && c.a.x0 == 0 && c.a.y1 == c.Ha && c.a.x1 == c.Wa, "%s: clip %d: packed taps need a full map a", who, i);
    }
    SLIC_REQUIRE(c.nops >= 0 && c.nops <= SLIC_CLIPTF_MAX_OPS, "%s: clip %d: %d colour ops", who, i, c.nops);
    int ncon = 0;
    for (int k = 0; k < c.nops; ++k) {
      SLIC_REQUIRE(c.op_kind[k] >= SLIC_CLIPTF_BRIGHTNESS && c.op_kind[k] <= SLIC_CLIPTF_GRAY, "%s: clip %d: unknown colour op", who, i);
      SLIC_REQUIRE(c.op_fac[k] >= 0 && (size_t)c.op_fac[k] >= first_fac && (size_t)c.op_fac[k] + N <= nfloat, "%s: clip %d: factor array outside the table", who, i);
      ncon += c.op_kind[k] == SLIC_CLIPTF_CONTRAST;
    }
    SLIC_REQUIRE(ncon <= 1, "%s: clip %d: more than one contrast op in a group", who, i);
    *any_contrast |= ncon;
  }
  return SLIC_OK;
}

template <bool STATS>
static void ct_launch(int kind, dim3 grid, void* stream, const char* table, int N, int Ho, int Wo, int normalize, int br, int nbands, float* ws,
                      float* out) {
  if (kind == SLIC_CLIPTF_SRC_U8)
    cliptf_kernel<SLIC_CLIPTF_SRC_U8, STATS><<<grid, dim3(CT_THREADS), 0, S_(stream)>>>(table, N, Ho, Wo, normalize, br, nbands, ws, out);
  else if (kind == SLIC_CLIPTF_SRC_U8_255)
    cliptf_kernel<SLIC_CLIPTF_SRC_U8_255, STATS><<<grid, dim3(CT_THREADS), 0, S_(stream)>>>(table, N, Ho, Wo, normalize, br, nbands, ws, out);
  else
    cliptf_kernel<SLIC_CLIPTF_SRC_F32, STATS><<<grid, dim3(CT_THREADS), 0, S_(stream)>>>(table, N, Ho, Wo, normalize, br, nbands, ws, out);
}

extern "C" size_t slic_clip_transform_workspace_bytes(int B, int N, int Ho, int Wo) {
  if (B <= 0 || N <= 0 || Ho <= 0 || Wo <= 0) return 0;
  return (size_t)B * N * slic_cdiv(Ho, ct_band_rows(Ho, Wo)) * sizeof(float);
}

extern "C" int slic_clip_transform_stats(const void* table, const void* table_host, size_t table_bytes, int B, int N, int Ho, int Wo, int kind,
                                         void* workspace, void* stream) {
  int any = 0;
  const int rc = ct_validate("slic_clip_transform_stats", table_host, table_bytes, B, N, Ho, Wo, kind, &any);
  if (rc != SLIC_OK) return rc;
  SLIC_REQUIRE(table && workspace, "slic_clip_transform_stats: NULL table or workspace");
  const int br = ct_band_rows(Ho, Wo), nbands = (int)slic_cdiv(Ho, br);
  ct_launch<true>(kind, dim3(nbands, N, B), stream, (const char*)table, N, Ho, Wo, 0, br, nbands, (float*)workspace, nullptr);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_clip_transform_apply(const void* table, const void* table_host, size_t table_bytes, int B, int N, int Ho, int Wo, int kind,
                                         int normalize, const void* workspace, float* out, void* stream) {
  int any = 0;
  const int rc = ct_validate("slic_clip_transform_apply", table_host, table_bytes, B, N, Ho, Wo, kind, &any);
  if (rc != SLIC_OK) return rc;
  SLIC_REQUIRE(table && out && ((uintptr_t)out & 15) == 0, "slic_clip_transform_apply: NULL table or out, or out not 16-byte aligned");
  SLIC_REQUIRE(!any || workspace, "slic_clip_transform_apply: a contrast op needs the workspace slic_clip_transform_stats filled");
  const int br = ct_band_rows(Ho, Wo), nbands = (int)slic_cdiv(Ho, br);
  ct_launch<false>(kind, dim3(nbands, N, B), stream, (const char*)table, N, Ho, Wo, normalize, br, nbands, (float*)workspace, out);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
