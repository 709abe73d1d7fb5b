// Certified bf16 candidate search for the cosine top-k (slic_cosine_topk_bf16): part of topk.hip, which includes this file after its own
// kernels and launch helpers (topk_stream, topk_thresholds, topk_select, the sample plan).
//
// The similarity GEMM of the collect path runs on v_mfma_f32_32x32x16_bf16 — 16 x the rate of the fp32 MFMA — and only NOMINATES rows:
//   1. tau_q: the fp32 sample pass of the collect path, unchanged (topk_partial_qreg on a strided sample + topk_thresholds);
//   2. tkb_convert: bf16 images (round to nearest even) of the normalised queries and gallery, rows zero-padded to Dp = D rounded up to 16;
//   3. topk_collect_bf16: the whole gallery against the queries on the bf16 MFMA; every row whose coarse score c >= tau_q - eps goes to
//      the query's candidate buffer with that score.  |c - s| <= eps (TK_BF16_EPS, derived in DESIGN.md) for the fp32 score s of unit
//      rows, so every row with s >= tau_q is a candidate;
//   4. topk_bf16_rescore: c_k = the k-th best coarse score of the query; a row of the true top-k has c >= c_k - 2 eps, so only those
//      candidates get their fp32 score, from the fp32 rows in a fixed summation order, and become (score, index) keys; the others are
//      struck.  The k best keys ARE the global top-k (the certificate; its second form, for a threshold close to c_k, is at the kernel)
//      and topk_select writes them out.  A query without it — fewer than k candidates, or more than its slots — goes on topk_select's
//      fallback list, and
//   5. topk_stream redoes the listed queries with the fp32 streaming kernels, as the fp32 collect path does.
// Nothing here is approximate in its result: the bf16 scores never reach the output.
#pragma once

#include "bf16_image.h"      // TK_BF16_EPS, tkb_round_bf16, tkb_convert: shared with the k-means E-step

#define TKB_PC 32             // pending candidates per lane between drains

// The collect pass on the bf16 MFMA.  The operand path is the register-operand ring of mfma_ring.h, byte for byte: a ring stage is
// 128 gallery rows x 128 BYTES — 64 bf16 columns instead of 32 floats — moved by the same DMAs into the same swizzled image, and the
// 16 bytes lane (r, h) reads at chunk 2 qd + h of its row are the 8 bf16 values v_mfma_f32_32x32x16_bf16 takes from that lane in MFMA
// step qd (k = 64 kt + 16 qd + 8 h + 0..7, the same for both operands).  Both images are therefore handled as rows of Df = Dp / 2
// "floats".  A wave holds its 32 queries in NK x 16 registers; one ds_read_b128 feeds one MFMA of 32 cycles, half of what the LDS
// array sustains beside the matrix pipe.  (Two query tiles per wave — one read per two MFMAs, half the L2 traffic — spilled at D = 512
// and measured 4-6 % slower at 10k x 100k x 512.)
// NK = k-tiles of 64 columns per row (4: D <= 256, 8: D <= 512; tiles past Dp are all-zero DMAs).
template <int NK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void topk_collect_bf16(
    const float* __restrict__ Qb, int Nq, const float* __restrict__ Gb, int Ng, int Df, int self_mask, int g_per_slice,
    const float* __restrict__ tau, float eps, int* __restrict__ cnt,
    unsigned long long* __restrict__ cand /* [Nq][cap]: {gallery index, coarse score bits} */, int cap) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(NK % 4 == 0, "a gallery tile is a whole number of ring turns");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // pending candidates: [4 waves][TKB_PC][64] pairs {gallery index, coarse score bits}, one column per LANE
  unsigned long long* pq = (unsigned long long*)(lds + 4 * SLIC_RT_TILE) + wave * TKB_PC * 64;
  const int q0 = blockIdx.x * TK_BQ;
  const int gbeg = blockIdx.y * g_per_slice;
  const int gend = min(gbeg + g_per_slice, Ng);
  int pc = 0;
  const int q = q0 + 32 * wave + r;
  // both halves of a lane pair serve query r and test against its lowered threshold; slots past Nq never see a candidate
  const float filt = q < Nq ? tau[q] - eps : INFINITY;
  f32x4 qr[NK][4];
  slic_rt_load_frags(qr, Qb + (int64_t)(q < Nq ? q : Nq - 1) * Df, Df, h);
  const SlicRtLane ln = slic_rt_lane(tid, Df);
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(Gb + (int64_t)gbeg * Df), 0, (int)((int64_t)(gend - gbeg) * Df * 4), 0x00020000);     // rows past the slice: zeros
  unsigned goff[4];
  slic_rt_offsets(goff, ln, (unsigned)Df * 4u);
  const int ntile = (gend - gbeg + TK_BG - 1) / TK_BG;
  auto issue = [&](int tile, int kt) SLIC_RT_INLINE {
    const bool live = ln.kin(kt) && tile < ntile;
    slic_rt_issue(rs_g, lds + (kt & 3) * SLIC_RT_TILE, wave, goff, (unsigned)tile * (unsigned)(TK_BG * Df * 4), kt, live);
  };
  // a lane's pending pairs -> the query's candidate buffer: one atomic add reserves the lane's slots (see topk_collect_qreg)
  auto drain = [&]() {
    if (pc > 0) {
      const int base = atomicAdd(cnt + q, pc);
      for (int j = 0; j < pc; ++j)
        if (base + j < cap) cand[(int64_t)q * cap + base + j] = pq[j * 64 + lane];
    }
    pc = 0;
  };
  f32x16 acc[4];
  f32x4 a[2][4];
  slic_rt_ring_prime<4>(a, lds, r, h, [&](int kn) SLIC_RT_INLINE { issue(0, kn); });
  for (int tile = 0; tile < ntile; ++tile) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ct][v] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
      // ring step s = (tile, kt), the contract of slic_rt_ring_ktile: step s + 1 has landed, the barrier publishes it and frees the
      // stage of step s - 1 for the DMAs of step s + 3
      slic_rt_wait<4>();
      __builtin_amdgcn_s_barrier();
      issue(kt + 3 >= NK ? tile + 1 : tile, kt + 3 >= NK ? kt + 3 - NK : kt + 3);
      slic_rt_ktile_mfma<false, 4, true>(acc, a, qr[kt], lds, kt & 3, r, h);
    }
    const int g0 = gbeg + tile * TK_BG;
    const bool ragged = g0 + TK_BG > gend;
    const bool selfhit = self_mask && g0 < q0 + 32 * wave + 32 && g0 + TK_BG > q0 + 32 * wave;
    const int gl = g0 + 4 * h;                                 // this lane's rows of the tile: gl + an immediate
    if (ragged || selfhit) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int gi = gl + ct * 32 + (v & 3) + 8 * (v >> 2);
          if (gi >= gend || (self_mask && gi == q)) acc[ct][v] = -INFINITY;      // never >= a finite threshold
        }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      if (__any(pc > TKB_PC - 16)) drain();                    // room for the sixteen scores of this accumulator in every lane's column
#pragma unroll
      for (int v0 = 0; v0 < 16; v0 += 4) {
        const float gm = fmaxf(fmaxf(acc[ct][v0], acc[ct][v0 + 1]), fmaxf(acc[ct][v0 + 2], acc[ct][v0 + 3]));
        if (gm >= filt) {
#pragma unroll
          for (int v = v0; v < v0 + 4; ++v)
            if (acc[ct][v] >= filt) {
              pq[pc * 64 + lane] = ((unsigned long long)(unsigned)(gl + (ct * 32 + (v & 3) + 8 * (v >> 2))) << 32) | __float_as_uint(acc[ct][v]);
              ++pc;
            }
        }
      }
    }
  }
  drain();
  slic_rt_wait<0>();                                           // the trailing all-zero DMAs must land before the workgroup leaves
}

// one WAVE per query: which of its n = cnt[q] candidates can still be among the k best, their fp32 scores, and the certificate.
//  * c_k, the k-th best COARSE score (a radix select over the order-preserving images, the candidates spread over the lanes' registers).
//    The k rows that reach it have s >= c_k - eps, so the k-th best fp32 score is >= c_k - eps, and a row of the top-k has
//    c >= s - eps >= c_k - 2 eps =: lo.  If lo >= tau - eps (the collect pass's threshold: every row with such a c WAS collected), only the
//    candidates with c >= lo are rescored and the k best of them are the global top-k — at k = 50 a quarter of the candidates.
//  * Otherwise (the sample's threshold came out close to c_k) every candidate is rescored and those with s >= tau are kept: every gallery
//    row with s >= tau has c >= tau - eps and was collected, so at least k of them again certify the k best.
//  * The fp32 score comes straight from the fp32 rows: 16 lanes share a candidate (lane `sub` takes columns 4 sub + 64 j .. + 3, a chain of
//    fused multiply-adds over j ascending, then a fixed butterfly over the 16 lanes), four candidates per round: the same bits on every
//    run, no float atomics.  A kept candidate becomes the (score, index) key of topk_select, any other is struck (key 0 sorts last).
//  * Fewer than k keys: cnt[q] is set past the cap, which is how topk_select recognises a query for the fallback list; an overflowed
//    query (n > cap) is left that way, n < k too.  tot[0] counts the queries that overflowed, tot[1] the candidates (integer atomics:
//    exact in any order).
#define TKB_PER (TKC_CAP / 64)                                 // candidates per lane
template <int NC>
__global__ __launch_bounds__(256) void topk_bf16_rescore(const float* __restrict__ Qn, const float* __restrict__ Gn, int Nq, int D, int k,
                                                         int cap, const float* __restrict__ tau, float eps, int* __restrict__ cnt,
                                                         unsigned long long* __restrict__ cand, int* __restrict__ tot) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Nq) return;                                         // (whole waves leave; nothing below needs the workgroup)
  const int n = cnt[q];
  if (n > cap || n < k) {
    if (lane == 0) { atomicAdd(tot, n > cap ? 1 : 0); atomicAdd(tot + 1, n > cap ? cap : n); }
    return;
  }
  unsigned long long* ck = cand + (int64_t)q * cap;
  // ---- c_k: the largest T with at least k images >= T, bit by bit (empty slots hold 0, below the image of every finite score)
  unsigned img[TKB_PER];
#pragma unroll
  for (int u = 0; u < TKB_PER; ++u) {
    const int e = lane + 64 * u;
    const unsigned b = e < n ? (unsigned)ck[e] : 0u;
    img[u] = e < n ? ((b & 0x80000000u) ? ~b : (b | 0x80000000u)) : 0u;
  }
  unsigned T = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned trial = T | (1u << bit);
    int c = 0;
#pragma unroll
    for (int u = 0; u < TKB_PER; ++u) c += img[u] >= trial ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (c >= k) T = trial;                                     // (wave-uniform)
  }
  const float ckth = __uint_as_float((T & 0x80000000u) ? (T & 0x7FFFFFFFu) : ~T);
  const float lo = ckth - 2.f * eps;
  const float tq = tau[q];
  const bool tight = lo >= tq - eps;                           // tq - eps: the expression topk_collect_bf16 tested the coarse scores against
  const float need_c = tight ? lo : -INFINITY, need_s = tight ? -INFINITY : tq;
  const int sub = lane & 15, grp = lane >> 4;
  f32x4 qv[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int col = 4 * sub + 64 * j;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    qv[j] = col < D ? *(const f32x4*)(Qn + (int64_t)q * D + col) : z;
  }
  int kept = 0;
  for (int i0 = 0; i0 < n; i0 += 4) {                          // (wave-uniform trip count: the shuffles below see all 64 lanes)
    const int i = i0 + grp;
    const bool valid = i < n;
    const unsigned long long raw = valid ? ck[i] : 0ull;
    const int gi = (int)(raw >> 32);
    const bool live = valid && __uint_as_float((unsigned)raw) >= need_c;       // (the same for the 16 lanes of a group)
    float s = 0.f;
    if (live) {
      const float* g = Gn + (int64_t)gi * D;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int col = 4 * sub + 64 * j;
        if (col < D) {
          const f32x4 gv = *(const f32x4*)(g + col);
          s = fmaf(qv[j][0], gv[0], s); s = fmaf(qv[j][1], gv[1], s); s = fmaf(qv[j][2], gv[2], s); s = fmaf(qv[j][3], gv[3], s);
        }
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (valid && sub == 0) {
      const bool keep = live && s >= need_s;
      ck[i] = keep ? tk_key(s, gi) : 0ull;
      kept += keep ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
  if (lane == 0) {
    atomicAdd(tot + 1, n);
    if (kept < k) cnt[q] = cap + 1;
  }
}

__global__ void topk_bf16_stats(const int* __restrict__ nfail, const int* __restrict__ tot, int32_t* __restrict__ stats) {
  stats[0] = *nfail; stats[1] = tot[0]; stats[2] = tot[1];
}

// SLIC_TOPK_BF16: 0 = never, 1 = wherever the shape is inside the collect path's domain (any k: the switch the tests use to reach k = 1),
// unset = where the bf16 pass measured faster than the fp32 path by more than that path's run-to-run spread (profiles/topk_bf16.txt).
struct TopkBf16Plan { bool on; TopkCollectPlan c; int Dp; };
static TopkBf16Plan topk_bf16_plan(int Nq, int Ng, int D, int k) {
  TopkBf16Plan p = {false, topk_collect_shape(Nq, Ng, k), (D + 15) / 16 * 16};
  const char* e = getenv("SLIC_TOPK_BF16");
  const bool domain = p.c.on && D > 0 && D <= 512 && D % 8 == 0 && (int64_t)Ng * D * 4 < (1ll << 31);
  const bool force = e && e[0] == '1', never = e && e[0] == '0';
  const bool measured = TKB_MEASURED_ON(Nq, Ng, D, k);
  p.on = domain && !never && (force || measured);
  return p;
}

static size_t topk_bf16_extra_bytes(const TopkBf16Plan& p, int Nq, int Ng) {
  return slic_align_up((size_t)Nq * p.Dp * 2, 256) + slic_align_up((size_t)Ng * p.Dp * 2, 256) + 256;
}

extern "C" float slic_cosine_topk_bf16_eps(void) { return TK_BF16_EPS; }

extern "C" size_t slic_cosine_topk_bf16_workspace_bytes(int Nq, int Ng, int D, int k) {
  if (Nq <= 0 || Ng <= 0 || D <= 0 || k < 1) return 0;
  const TopkBf16Plan p = topk_bf16_plan(Nq, Ng, D, k);
  if (!p.on) return slic_cosine_topk_workspace_bytes(Nq, Ng, k);
  return topk_stream_bytes(Nq, Ng, k) + topk_collect_bytes(p.c, Nq) + topk_bf16_extra_bytes(p, Nq, Ng);
}

extern "C" int slic_cosine_topk_bf16_plan(int Nq, int Ng, int D, int k, int* out) {
  SLIC_REQUIRE(out && Nq > 0 && Ng > 0 && D > 0 && k >= 1, "slic_cosine_topk_bf16_plan: bad args");
  const TopkBf16Plan p = topk_bf16_plan(Nq, Ng, D, k);
  out[0] = p.on ? 1 : 0; out[1] = p.on ? p.c.cap : 0; out[2] = p.on ? p.Dp : 0; out[3] = p.on ? TK_BQ : 0;
  out[4] = p.on ? p.c.S1 * p.c.per1 : 0; out[5] = p.on ? p.c.m1 : 0;
  return SLIC_OK;
}

extern "C" int slic_cosine_topk_bf16(const float* Qn, int Nq, const float* Gn, int Ng, int D, int k, int self_mask, int32_t* out_idx,
                                     float* out_dist, int32_t* stats, void* workspace, void* stream) {
  SLIC_REQUIRE(Qn && Gn && out_idx && out_dist && workspace, "slic_cosine_topk_bf16: null pointer");
  SLIC_REQUIRE(Nq > 0 && Ng > 0 && D > 0 && D % 8 == 0 && k >= 1 && k <= TK_KMAX && k <= Ng,
               "slic_cosine_topk_bf16: need D %% 8 == 0, 1 <= k <= min(%d, Ng) (Nq=%d Ng=%d D=%d k=%d)", TK_KMAX, Nq, Ng, D, k);
  SLIC_REQUIRE(((uintptr_t)Qn % 16) == 0 && ((uintptr_t)Gn % 16) == 0, "slic_cosine_topk_bf16: unaligned");
  hipStream_t st = S_(stream);
  const TopkBf16Plan p = topk_bf16_plan(Nq, Ng, D, k);
  if (!p.on) {                                                 // outside the measured domain the call IS the fp32 search
    if (stats) SLIC_HIP_CHECK(hipMemsetAsync(stats, 0, 3 * sizeof(int32_t), st));
    return slic_cosine_topk(Qn, Nq, Gn, Ng, D, k, self_mask, out_idx, out_dist, workspace, stream);
  }
  const TopkCollectPlan& c = p.c;
  SlicCarver w(workspace);
  float* pval1 = w.take<float>((size_t)c.S1 * Nq * c.ms);
  int32_t* pidx1 = w.take<int32_t>((size_t)c.S1 * Nq * c.ms);
  float* tau = w.take<float>((size_t)Nq);
  int* cnt = w.take<int>((size_t)Nq);
  int* failq = w.take<int>((size_t)Nq);
  int* nfail = w.take<int>(64);
  unsigned long long* cand = w.take<unsigned long long>((size_t)Nq * c.cap);
  float* Qb = (float*)w.take<uint16_t>((size_t)Nq * p.Dp);
  float* Gb = (float*)w.take<uint16_t>((size_t)Ng * p.Dp);
  int* tot = w.take<int>(64);
  const bool same = Qn == Gn && Nq == Ng;                      // the self search: one image serves both operands
  SLIC_HIP_CHECK(hipMemsetAsync(tot, 0, 2 * sizeof(int), st));
  // ---- 1. tau_q and cnt_q = 0 from the fp32 sample
  const int rc1 = topk_sample_thresholds<false>(c, Qn, Nq, Gn, D, nullptr, pval1, pidx1, tau, cnt, nfail, st);
  if (rc1) return rc1;
  // ---- 2. the bf16 images
  const int cpr = p.Dp / 8;
  tkb_convert<<<dim3((unsigned)slic_cdiv((int64_t)Ng * cpr, 256)), dim3(256), 0, st>>>(Gn, Ng, D, D, p.Dp, (uint4*)Gb);
  SLIC_LAUNCH_CHECK();
  if (same) Qb = Gb;
  else {
    tkb_convert<<<dim3((unsigned)slic_cdiv((int64_t)Nq * cpr, 256)), dim3(256), 0, st>>>(Qn, Nq, D, D, p.Dp, (uint4*)Qb);
    SLIC_LAUNCH_CHECK();
  }
  // ---- 3. the whole gallery on the bf16 MFMA against tau - eps
  {
    const int slices = topk_slices(Nq, Ng, 0);
    int per = (int)slic_cdiv(Ng, slices);
    per = (int)slic_cdiv(per, TK_BG) * TK_BG;
    const int S = (int)slic_cdiv(Ng, per);
    const size_t lds = (size_t)4 * SLIC_RT_TILE * sizeof(float) + (size_t)4 * TKB_PC * 64 * sizeof(unsigned long long);
    const int Df = p.Dp / 2;
    const auto kern = p.Dp > 256 ? topk_collect_bf16<8> : topk_collect_bf16<4>;
    SLIC_LDS_LIMIT(kern, lds);
    kern<<<dim3((unsigned)slic_cdiv(Nq, TK_BQ), (unsigned)S), dim3(256), lds, st>>>(Qb, Nq, Gb, Ng, Df, self_mask, per, tau, TK_BF16_EPS, cnt, cand, c.cap);
    SLIC_LAUNCH_CHECK();
  }
  // ---- 4. exact scores of the candidates, the certificate, the k best; 5. the uncertified queries through the fp32 streaming kernels
  {
    const auto kern = D > 256 ? topk_bf16_rescore<8> : D > 128 ? topk_bf16_rescore<4> : topk_bf16_rescore<2>;
    kern<<<dim3((unsigned)slic_cdiv(Nq, 4)), dim3(256), 0, st>>>(Qn, Gn, Nq, D, k, c.cap, tau, TK_BF16_EPS, cnt, cand, tot);
    SLIC_LAUNCH_CHECK();
  }
  topk_select<true><<<dim3((unsigned)slic_cdiv(Nq, TKS_WAVES)), dim3(64 * TKS_WAVES), 0, st>>>(cand, cnt, Nq, k, c.cap, out_idx, out_dist, failq, nfail);
  SLIC_LAUNCH_CHECK();
  if (stats) {
    topk_bf16_stats<<<dim3(1), dim3(1), 0, st>>>(nfail, tot, stats);
    SLIC_LAUNCH_CHECK();
  }
  return topk_stream<false>(Qn, Nq, Gn, Ng, D, k, self_mask, out_idx, out_dist, nullptr, w, st, failq, nfail);
}
