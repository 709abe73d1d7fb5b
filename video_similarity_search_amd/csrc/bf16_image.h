// bf16 images for the certified candidate passes: the cosine top-k (topk_bf16.h) and the k-means E-step (kmeans.hip) both run their
// GEMM on v_mfma_f32_32x32x16_bf16 over round-to-nearest-even images of the fp32 rows and only NOMINATE with it.  One copy of the
// rounding, of the image kernel and of the error constant (derived in DESIGN.md).
#pragma once
#include "common.h"

// |bf16-MFMA dot (fp32 accumulation) - fp32 dot| <= TK_BF16_EPS * ||x|| * ||c|| for D <= 512: the proven constant is 0.007951
#define TK_BF16_EPS 0.008f

typedef __bf16 tkb_bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned tkb_round_bf16(float x) {
  const unsigned u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;                          // NaN stays NaN
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;                                // round to nearest, ties to even
}

// one thread per 16-byte chunk of the image: 8 consecutive columns of a row (D % 8 == 0: a chunk is inside the row or in the padding).
// Source rows are ldx floats apart; image rows are dense, Dp = D rounded up to 16 columns, the padding zero.  (static: one copy per
// translation unit that includes this header.)
static __global__ __launch_bounds__(256) void tkb_convert(const float* __restrict__ X, int64_t N, int D, int64_t ldx, int Dp, uint4* __restrict__ out) {
  const int cpr = Dp >> 3;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * cpr) return;
  const int64_t row = e / cpr;
  const int c = (int)(e - row * cpr) * 8;
  uint4 o = {0u, 0u, 0u, 0u};
  if (c < D) {
    const f32x4 a = *(const f32x4*)(X + row * ldx + c), b = *(const f32x4*)(X + row * ldx + c + 4);
    o.x = tkb_round_bf16(a[0]) | (tkb_round_bf16(a[1]) << 16);
    o.y = tkb_round_bf16(a[2]) | (tkb_round_bf16(a[3]) << 16);
    o.z = tkb_round_bf16(b[0]) | (tkb_round_bf16(b[1]) << 16);
    o.w = tkb_round_bf16(b[2]) | (tkb_round_bf16(b[3]) << 16);
  }
  out[e] = o;
}
