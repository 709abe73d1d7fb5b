// Classifier head (the reference's coclr_classify.py on models/resnet.py:192-201, 305-307): general-target softmax cross-entropy with
// the rank of the target logit from the same pass (top-1 / top-5 hit counts, coclr_utils/utils.py:55-75), its backward, and a
// counter-based dropout whose mask is recomputed, not stored.
//
//   softmax_ce_fwd_kernel : one wave per row, strided over the C logits (any C; rows independent).  Pass 1 the row maximum, pass 2
//                           sum exp(x - max) and the rank count; the row's loss is log(sum) - (x_t - max), the form
//                           torch's log_softmax takes: x_t - max is exact or nearly so, and no term of size |max| is rounded.
//   ce_finish_kernel      : one workgroup: mean of the row losses (fp64 accumulation, fixed order), top-1 / top-5 hit counts and
//                           the number of rows whose target is outside [0, C) — the host wrapper reads that flag; such a row is
//                           never dereferenced.
//   softmax_ce_bwd_kernel : (softmax - onehot) * gscale / B, one thread per element.
//   dropout_kernel        : Philox4x32-10 (Salmon et al., SC'11) keyed by seed, counter = (element index / 4, offset); four
//                           uniforms per counter serve four consecutive elements.  Forward and backward are the same map
//                           v -> keep ? v / (1 - p) : 0 (p = 1 keeps nothing).  torch's own dropout stream is NOT reproduced.
#include "common.h"
#include <math.h>


__global__ __launch_bounds__(256) void softmax_ce_fwd_kernel(const float* __restrict__ x, int64_t ld, int B, int C,
                                                             const int64_t* __restrict__ tgt, float* __restrict__ lse,
                                                             float* __restrict__ rowloss, int32_t* __restrict__ rank) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const int lane = threadIdx.x & 63;
  const float* r = x + (int64_t)row * ld;
  const int64_t t = tgt[row];
  const bool ok = t >= 0 && t < (int64_t)C;
  float m = -INFINITY;
  for (int j = lane; j < C; j += 64) m = fmaxf(m, r[j]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  const float xt = ok ? r[t] : 0.f;
  float s = 0.f;
  int cnt = 0;
  for (int j = lane; j < C; j += 64) {
    const float v = r[j];
    s += expf(v - m);
    cnt += (ok && (v > xt || (v == xt && (int64_t)j < t))) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); cnt += __shfl_xor(cnt, o); }
  if (lane == 0) {
    const float ls = logf(s);
    lse[2 * (int64_t)row] = m;
    lse[2 * (int64_t)row + 1] = ls;
    rowloss[row] = ok ? ls - (xt - m) : 0.f;
    rank[row] = ok ? cnt : -1;
  }
}

__global__ __launch_bounds__(256) void ce_finish_kernel(const float* __restrict__ rowloss, const int32_t* __restrict__ rank, int B,
                                                        float* __restrict__ loss, int32_t* __restrict__ head) {
  __shared__ double sa[4];
  __shared__ int s1[4], s5[4], sb[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double a = 0.0;
  int h1 = 0, h5 = 0, bad = 0;
  for (int i = t; i < B; i += 256) {
    const int rk = rank[i];
    a += (double)rowloss[i];
    bad += rk < 0;
    h1 += rk == 0;
    h5 += rk >= 0 && rk < 5;
  }
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o); h1 += __shfl_xor(h1, o); h5 += __shfl_xor(h5, o); bad += __shfl_xor(bad, o);
  }
  if (lane == 0) { sa[wave] = a; s1[wave] = h1; s5[wave] = h5; sb[wave] = bad; }
  __syncthreads();
  if (t == 0) {
    const int nb = sb[0] + sb[1] + sb[2] + sb[3];
    head[0] = nb;
    head[1] = s1[0] + s1[1] + s1[2] + s1[3];
    head[2] = s5[0] + s5[1] + s5[2] + s5[3];
    *loss = nb ? NAN : (float)((((sa[0] + sa[1]) + sa[2]) + sa[3]) / (double)B);
  }
}

__global__ __launch_bounds__(256) void softmax_ce_bwd_kernel(const float* __restrict__ x, int64_t ld, const float* __restrict__ lse,
                                                             const int64_t* __restrict__ tgt, int B, int C,
                                                             const float* __restrict__ gscale, float* __restrict__ dx) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * C) return;
  const int64_t b = idx / C;
  const int64_t j = idx - b * C;
  const float g = (gscale ? *gscale : 1.f) / (float)B;
  const float p = expf((x[b * ld + j] - lse[2 * b]) - lse[2 * b + 1]);
  dx[idx] = (p - (j == tgt[b] ? 1.f : 0.f)) * g;
}

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// one thread per group of four consecutive elements; vec: both pointers 16-byte aligned
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, int64_t n, float p, float keepp, uint64_t seed,
                                                      uint64_t offset, int vec, float* __restrict__ y) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t i0 = q * 4;
  if (i0 >= n) return;
  uint32_t c[4] = {(uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  float k[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) k[e] = ((float)(c[e] >> 8) * (1.0f / 16777216.0f)) >= p ? 1.f : 0.f;     // uniform in [0, 1): keep with probability keepp = 1 - p
  if (vec && i0 + 4 <= n) {
    const f32x4 v = *(const f32x4*)(x + i0);
    f32x4 o;
    o[0] = k[0] != 0.f ? v[0] / keepp : 0.f;
    o[1] = k[1] != 0.f ? v[1] / keepp : 0.f;
    o[2] = k[2] != 0.f ? v[2] / keepp : 0.f;
    o[3] = k[3] != 0.f ? v[3] / keepp : 0.f;
    *(f32x4*)(y + i0) = o;
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i0 + e < n) y[i0 + e] = k[e] != 0.f ? x[i0 + e] / keepp : 0.f;       // a dropped inf / nan is 0, as torch's masked form
}

static int dropout_launch(const char* who, const float* x, int64_t n, float p, uint64_t seed, uint64_t offset, float* y, void* stream) {
  SLIC_REQUIRE(x && y && n > 0 && p >= 0.f && p <= 1.f, "%s: bad args (0 <= p <= 1, n > 0)", who);
  SLIC_REQUIRE(slic_cdiv(n, 4 * 256) < ((int64_t)1 << 31), "%s: n too large for one launch", who);
  const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  dropout_kernel<<<dim3((unsigned)slic_cdiv(n, 4 * 256)), dim3(256), 0, S_(stream)>>>(x, n, p, 1.0f - p, seed, offset, vec, y);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_dropout_fwd(const float* x, int64_t n, float p, uint64_t seed, uint64_t offset, float* y, void* stream) {
  return dropout_launch("slic_dropout_fwd", x, n, p, seed, offset, y, stream);
}

extern "C" int slic_dropout_bwd(const float* dy, int64_t n, float p, uint64_t seed, uint64_t offset, float* dx, void* stream) {
  return dropout_launch("slic_dropout_bwd", dy, n, p, seed, offset, dx, stream);
}

extern "C" int slic_softmax_ce_fwd(const float* logits, int64_t ld, int B, int C, const int64_t* targets, float* lse, float* rowloss,
                                   float* loss, int32_t* topk_hits, void* stream) {
  SLIC_REQUIRE(logits && targets && lse && rowloss && loss && topk_hits && B > 0 && C > 0 && ld >= (int64_t)C,
               "slic_softmax_ce_fwd: bad args (B, C > 0, ld >= C)");
  softmax_ce_fwd_kernel<<<dim3((unsigned)slic_cdiv(B, 4)), dim3(256), 0, S_(stream)>>>(logits, ld, B, C, targets, lse, rowloss,
                                                                                       topk_hits + SLIC_CE_HITS_HEAD);
  SLIC_LAUNCH_CHECK();
  ce_finish_kernel<<<dim3(1), dim3(256), 0, S_(stream)>>>(rowloss, topk_hits + SLIC_CE_HITS_HEAD, B, loss, topk_hits);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_softmax_ce_bwd(const float* logits, int64_t ld, const float* lse, const int64_t* targets, int B, int C,
                                   const float* gscale, float* dlogits, void* stream) {
  SLIC_REQUIRE(logits && lse && targets && dlogits && B > 0 && C > 0 && ld >= (int64_t)C, "slic_softmax_ce_bwd: bad args (B, C > 0, ld >= C)");
  softmax_ce_bwd_kernel<<<dim3((unsigned)slic_cdiv((int64_t)B * C, 256)), dim3(256), 0, S_(stream)>>>(logits, ld, lse, targets, B, C,
                                                                                                     gscale, dlogits);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
