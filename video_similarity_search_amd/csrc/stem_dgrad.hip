// Data gradient of the stem convolution (kt x 7 x 7, stride (st, 2, 2), pad (kt / 2, 3, 3), C <= 4 input channels): the gradient
// with respect to the CLIP, written in the clip's own NCDHW layout.  What autograd derives for nn.Conv3d's input in the reference
// (models/resnet.py:126-131, 255-261) when the clip requires a gradient: saliency maps, adversarial probes, a learnable module in
// front of the encoder.
//
// Formulation: one GEMM row per COARSE position (b, t, hc = h / 2, wc = w / 2), one column per (channel, h parity, w parity) —
// C x 2 x 2 <= 16 columns, the width of v_mfma_f32_16x16x4_f32 — and K = (kt taps) x (4 h offsets x 4 w offsets into dz) x N.
// An input row h = 2 hc + qh receives dz[ho = hc + oh] through tap dh = qh + 3 - 2 oh: parity 0 has taps 5, 3, 1 at offsets
// -1, 0, 1, parity 1 has taps 6, 4, 2, 0 at offsets -1 .. 2; the packed weight operand is zero where a parity class has no tap
// (and in the columns past 4 C).  The t axis is not folded: a row's t is the fine t, and the taps dt with (t + pt - dt) % st != 0
// or with their dz plane outside [0, To) are skipped — t is uniform per workgroup, so the skip is a uniform branch.
//
// A workgroup (4 waves) owns one (b, t) and a patch of 8 x 16 coarse positions; wave w computes the two 16-position row tiles of
// coarse rows 2 w, 2 w + 1.  Per stage (one dt, one chunk of NC <= 32 channels of dz) the patch's halo — (8 + 3) x (16 + 3)
// positions of dz, zeros outside the tensor — and the 16 offsets' weight operand go through LDS: 30 KB + 32 KB, two workgroups
// per CU; the next stage's chunks are fetched into registers under the current stage's MFMAs.  Position stride NC + 4 floats:
// the 16 rows of a ds_read_b64 half-wave land on 16 different 16-byte slots (NC % 8 == 0 => (NC + 4) / 4 is odd).
// Exact fp32: every output element is one fixed-order chain of fmaf (dt ascending, channel chunk, offset, channel); no atomics.
#include "common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

#define SD_PH 8                      // coarse rows of a patch
#define SD_PW 16                     // coarse columns of a patch = rows of one MFMA tile
#define SD_NC 32                     // channels of dz per stage (at most)
#define SD_HP (SD_PH + 3)            // halo: offsets -1 .. 2
#define SD_WP (SD_PW + 3)
#define SD_THREADS 256

struct StemDgradArgs {
  const float* dz;
  const float* wp;
  float* dx;
  int B, C, T, H, W, To, Ho, Wo, N, kt, st, NC, nPh, nPw;
};

static inline int sd_chunk(int N) {                  // largest multiple of 8 that divides N and fits a stage
  for (int nc = SD_NC; nc > 8; nc -= 8)
    if (N % nc == 0) return nc;
  return 8;
}

// Wp[dt][off = 4 (oh + 1) + (ow + 1)][g = n / 8][kq][j][m], n = 8 g + 2 kq + m, column j = 4 c + 2 qh + qw: the order in which a
// lane (j = lane & 15, kq = lane >> 4) reads its two B values of channel group g as one 8-byte word
__global__ void stem_dgrad_pack_kernel(const float* __restrict__ W, int N, int C, int kt, float* __restrict__ Wp) {
  const int64_t tot = (int64_t)kt * 16 * N * 16;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= tot) return;
  const int m = (int)(e & 1), j = (int)((e >> 1) & 15), kq = (int)((e >> 5) & 3);
  int64_t r = e >> 7;
  const int G = N / 8;
  const int g = (int)(r % G);
  r /= G;
  const int off = (int)(r & 15), dt = (int)(r >> 4);
  const int n = 8 * g + 2 * kq + m;
  const int c = j >> 2, qh = (j >> 1) & 1, qw = j & 1;
  const int dh = qh + 3 - 2 * ((off >> 2) - 1), dw = qw + 3 - 2 * ((off & 3) - 1);
  float v = 0.f;
  if (c < C && dh >= 0 && dh < 7 && dw >= 0 && dw < 7) v = W[(((int64_t)n * C + c) * kt + dt) * 49 + dh * 7 + dw];
  Wp[e] = v;
}

#define SD_A_IT ((SD_HP * SD_WP * (SD_NC / 4) + SD_THREADS - 1) / SD_THREADS)      // 16-byte chunks of a stage per thread: dz halo
#define SD_B_IT (16 * SD_NC * 4 / SD_THREADS)                                      // ... and weight operand

__global__ __launch_bounds__(SD_THREADS) void stem_dgrad_kernel(StemDgradArgs a) {
  extern __shared__ float sd_lds[];
  const int NC = a.NC, S = NC + 4;
  float* As = sd_lds;                                // [SD_HP * SD_WP positions][S]
  float* Bs = sd_lds + SD_HP * SD_WP * S;            // [16 offsets][NC / 8][4 kq][16 j][2]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, kq = lane >> 4;
  int blk = blockIdx.x;
  const int wc0 = (blk % a.nPw) * SD_PW;
  blk /= a.nPw;
  const int hc0 = (blk % a.nPh) * SD_PH;
  blk /= a.nPh;
  const int t = blk % a.T, b = blk / a.T;
  const int pt = a.kt / 2;
  const int G = NC / 8, Q = NC / 4;
  f32x4 acc[2];
  acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int Hc = (a.H + 1) >> 1;
  const bool wave_live = hc0 + 2 * wave < Hc;        // both row tiles of this wave lie below the clip: nothing to compute or store

  // What this thread moves per stage is the same every stage up to the (dt, n0) base: chunk e = tid + 256 k of the halo is
  // channels 4 ch .. of position pos; of the weight operand, chunk e lands at float 4 e of the LDS image.
  int a_src[SD_A_IT], a_dst[SD_A_IT];                // float offsets into the dz plane (-1: zeros) / into As (-1: no such chunk)
  int b_src[SD_B_IT];                                // float offset into the (dt, n0) block of Wp (-1: no such chunk)
#pragma unroll
  for (int k = 0; k < SD_A_IT; ++k) {
    const int e = tid + SD_THREADS * k;
    const int pos = e / Q, ch = e - pos * Q;
    const int ph = pos / SD_WP, pw = pos - ph * SD_WP;
    const int ho = hc0 - 1 + ph, wo = wc0 - 1 + pw;
    a_dst[k] = pos < SD_HP * SD_WP ? pos * S + 4 * ch : -1;
    a_src[k] = (pos < SD_HP * SD_WP && ho >= 0 && ho < a.Ho && wo >= 0 && wo < a.Wo) ? (ho * a.Wo + wo) * a.N + 4 * ch : -1;
  }
#pragma unroll
  for (int k = 0; k < SD_B_IT; ++k) {
    const int e = tid + SD_THREADS * k;
    const int off = e / (NC * 4);
    b_src[k] = e < 16 * NC * 4 ? 4 * e + off * (a.N - NC) * 16 : -1;
  }

  // stages: the taps dt whose dz plane exists for this t, times the channel chunks; the next stage's chunks are fetched into
  // registers under the current stage's MFMAs
  auto next_dt = [&](int dt) {
    for (; dt < a.kt; ++dt) {
      const int num = t + pt - dt;
      if (num >= 0 && num % a.st == 0 && num / a.st < a.To) break;
    }
    return dt;
  };
  f32x4 ra[SD_A_IT], rb[SD_B_IT];
  auto fetch = [&](int dt, int n0) {
    const int to = (t + pt - dt) / a.st;
    const float* plane = a.dz + ((int64_t)b * a.To + to) * a.Ho * a.Wo * a.N + n0;
    const float* wblk = a.wp + ((int64_t)dt * 16 * a.N + n0) * 16;
#pragma unroll
    for (int k = 0; k < SD_A_IT; ++k) {
      ra[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (a_src[k] >= 0) ra[k] = *(const f32x4*)(plane + a_src[k]);
    }
#pragma unroll
    for (int k = 0; k < SD_B_IT; ++k)
      if (b_src[k] >= 0) rb[k] = *(const f32x4*)(wblk + b_src[k]);
  };
  int dt = next_dt(0), n0 = 0;
  if (dt < a.kt) fetch(dt, n0);
  while (dt < a.kt) {
    __syncthreads();                                 // the previous stage has been read
#pragma unroll
    for (int k = 0; k < SD_A_IT; ++k)
      if (a_dst[k] >= 0) *(f32x4*)&As[a_dst[k]] = ra[k];
#pragma unroll
    for (int k = 0; k < SD_B_IT; ++k)
      if (b_src[k] >= 0) *(f32x4*)&Bs[4 * (tid + SD_THREADS * k)] = rb[k];
    __syncthreads();
    n0 += NC;
    if (n0 >= a.N) {
      n0 = 0;
      dt = next_dt(dt + 1);
    }
    if (dt < a.kt) fetch(dt, n0);
    if (!wave_live) continue;
#pragma unroll 4
    for (int off = 0; off < 16; ++off) {
      const float* ap = As + ((2 * wave + (off >> 2)) * SD_WP + i + (off & 3)) * S + 2 * kq;
      const float* bp = Bs + off * NC * 16 + kq * 32 + 2 * i;
      for (int g = 0; g < G; ++g) {
        const f32x2 bv = *(const f32x2*)(bp + g * 128);
        const f32x2 a0 = *(const f32x2*)(ap + 8 * g);
        const f32x2 a1 = *(const f32x2*)(ap + SD_WP * S + 8 * g);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bv.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, bv.x, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bv.y, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, bv.y, acc[1], 0, 0, 0);
      }
    }
  }

  // acc[r][v] = dx at coarse (hc0 + 2 wave + r, wc0 + 4 kq + v), column i = 4 c + 2 qh + qw.  The two w parities sit on
  // neighbouring lanes: they trade halves, so that a lane holds four consecutive w of one row of the clip.
  const int c = i >> 2, qh = (i >> 1) & 1, qw = i & 1;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const float s0 = qw ? acc[r][0] : acc[r][2], s1 = qw ? acc[r][1] : acc[r][3];
    const float g0 = __shfl_xor(s0, 1), g1 = __shfl_xor(s1, 1);
    float o[4];
    if (qw == 0) { o[0] = acc[r][0]; o[1] = g0; o[2] = acc[r][1]; o[3] = g1; }
    else         { o[0] = g0; o[1] = acc[r][2]; o[2] = g1; o[3] = acc[r][3]; }
    const int h = 2 * (hc0 + 2 * wave + r) + qh;
    const int w0 = 2 * (wc0 + 4 * kq + 2 * qw);
    if (c < a.C && h < a.H) {
      float* row = a.dx + ((((int64_t)b * a.C + c) * a.T + t) * a.H + h) * a.W;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (w0 + u < a.W) row[w0 + u] = o[u];
    }
  }
}

extern "C" int slic_pack_weight_stem_dgrad(const float* W, int N, int C, int kt, float* Wp, void* stream) {
  SLIC_REQUIRE(W && Wp, "slic_pack_weight_stem_dgrad: null pointer");
  SLIC_REQUIRE(N > 0 && N % 8 == 0 && C >= 1 && C <= 4 && kt >= 1 && kt <= 7 && (kt & 1),
               "slic_pack_weight_stem_dgrad: N %% 8 == 0, 1 <= C <= 4, kt odd <= 7 (got N %d, C %d, kt %d)", N, C, kt);
  const int64_t tot = (int64_t)kt * 16 * N * 16;
  stem_dgrad_pack_kernel<<<dim3((unsigned)slic_cdiv(tot, 256)), dim3(256), 0, S_(stream)>>>(W, N, C, kt, Wp);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_conv_stem_dgrad(const float* dz, const float* Wp, int B, int C, int T, int H, int W, int N, int kt, int st,
                                    float* dx, void* stream) {
  SLIC_REQUIRE(dz && Wp && dx, "slic_conv_stem_dgrad: null pointer");
  SLIC_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0, "slic_conv_stem_dgrad: empty clip");
  SLIC_REQUIRE(N > 0 && N % 8 == 0 && C >= 1 && C <= 4 && kt >= 1 && kt <= 7 && (kt & 1) && (st == 1 || st == 2),
               "slic_conv_stem_dgrad: kt x 7 x 7 / (st, 2, 2) with N %% 8 == 0, 1 <= C <= 4, kt odd <= 7, st 1 or 2 "
               "(got N %d, C %d, kt %d, st %d)", N, C, kt, st);
  SLIC_REQUIRE(((uintptr_t)dz % 16) == 0 && ((uintptr_t)Wp % 16) == 0, "slic_conv_stem_dgrad: dz and Wp must be 16-byte aligned");
  StemDgradArgs a;
  a.dz = dz; a.wp = Wp; a.dx = dx;
  a.B = B; a.C = C; a.T = T; a.H = H; a.W = W; a.N = N; a.kt = kt; a.st = st;
  a.To = (T - 1) / st + 1;                           // (T + 2 (kt / 2) - kt) / st + 1
  a.Ho = (H - 1) / 2 + 1;
  a.Wo = (W - 1) / 2 + 1;
  a.NC = sd_chunk(N);
  a.nPh = (int)slic_cdiv((H + 1) / 2, SD_PH);
  a.nPw = (int)slic_cdiv((W + 1) / 2, SD_PW);
  const int64_t wgs = (int64_t)B * T * a.nPh * a.nPw;
  SLIC_REQUIRE((int64_t)a.Ho * a.Wo * N < (1ll << 31), "slic_conv_stem_dgrad: one plane of dz exceeds 2^31 elements");
  SLIC_REQUIRE(wgs < (1ll << 31), "slic_conv_stem_dgrad: %lld workgroups exceed one launch (split the batch)", (long long)wgs);
  const size_t lds = ((size_t)SD_HP * SD_WP * (a.NC + 4) + (size_t)16 * a.NC * 16) * sizeof(float);
  SLIC_LDS_LIMIT(stem_dgrad_kernel, lds);
  stem_dgrad_kernel<<<dim3((unsigned)wgs), dim3(SD_THREADS), lds, S_(stream)>>>(a);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
