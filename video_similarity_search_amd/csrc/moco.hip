// MoCo queue contrast (loss/NCE_loss.py MemoryMoCo; the InfoNCE / UberNCE loss): one batch of queries q [B, D] against a dense queue
// memory [K, D], softmax against column 0 (and, with labels, against every queue row of the query's class).
//   logit[b, 0] = <q_b, k_b> / T,  logit[b, 1 + j] = <memory_j, q_b> / T
// All arithmetic is exact fp32 on v_mfma_f32_32x32x2_f32 (the positive column: vector FMAs); no float atomics; every sum has a fixed
// order, so two runs give the same bits.
//
// Two tile engines share the epilogues:
//  * moco_ring (forward, D % 4 == 0): the register-operand ring of mfma_ring.h, as topk_collect_qreg runs it.  A workgroup keeps 128
//    query rows in registers (32 per wave, NK * 16 registers per lane) and streams its slice of the queue ONCE through the 4-stage LDS
//    ring, 128 rows a tile.  After a tile, lane (r, h) of wave w holds the logits of query 32 w + r against the tile's rows
//    32 ct + 8 i + 4 h + j (acc[ct][4 i + j]).  LOGITS: they are stored.  CE: they feed the lane's online (max, sum-exp) pair (and, with
//    labels, the sum and count of its positives); the two lane halves merge at the end: one record per (K-slice, query).
//  * moco_tile32 (backward, and the forward of a D the DMA cannot address: D % 4 != 0): 32 queries x 128 queue rows per step,
//    operands loaded from memory (the queue tile comes from L2 when it is read the second time).  Wave w multiplies the queue rows
//    32 w .. 32 w + 31 by the 32 queries; for a backward the coefficient tile c [128 rows][32 queries] (CE: softmax - w, recomputed
//    from the saved lse; LOGITS: the incoming gradient) goes through LDS and wave w accumulates dq^T [d, q] for its share of the d-tiles
//    over the 128 rows: dq_partial[slice][q][d].  moco_dq_reduce adds the slices in ascending order, the positive column's term and
//    the scale.
// The fused step holds no [B, K] and no [K, D] temporary: its workspace is SLIC_MOCO_PARTS records per query and SLIC_MOCO_DQ_PARTS
// partial gradients.
//
// Rank of the best positive (slic_moco_topk_hits: the top-k accuracy of the step) runs on the same two engines as two more epilogues,
// two sweeps over the queue: BEST keeps the lane's first positive column in (descending logit, ascending column) order, COUNT counts
// the columns ahead of the row's winner.  Both sweeps form the same accumulators in the same order, so a logit has the same bits in
// both; the records are (float, int) pairs and integer counts, merged in any order with the same result.  Without labels column 0 is
// the only positive and the first sweep is not run.
#include <limits.h>
#include <math.h>
#include <type_traits>
#include "mfma_ring.h"

#define MOCO_BG 128                    // queue rows per tile
#define MOCO_CS_LD 33                  // row pitch of the coefficient tile in LDS (32 queries + 1: the transposing fill stays conflict-free)

enum { MOCO_LOGITS = 0, MOCO_CE = 1, MOCO_CE_BWD = 2, MOCO_LOGITS_BWD = 3, MOCO_BEST = 4, MOCO_COUNT = 5 };

// a column of the logit matrix as the rank orders them: descending logit, ties by ascending column.  v: the logit's bits
struct MocoCol { float v; int c; };
static_assert(sizeof(MocoCol) == 8, "one 8-byte record");
__device__ __forceinline__ bool moco_ahead(float v, int c, float v2, int c2) { return v > v2 || (v == v2 && c < c2); }

// queue row of accumulator register v, relative to the lane's first one (MFMA 32x32 output layout)
__device__ __forceinline__ int moco_vrow(int v) { return (v & 3) + 8 * (v >> 2); }

__device__ __forceinline__ bool moco_is_pos(int64_t ql, int64_t lq) { return ql >= 0 && ql == lq; }

// (m, s) <- merge with (m2, s2): s counts exp(x - m)
__device__ __forceinline__ void moco_merge(float& m, float& s, float m2, float s2) {
  const float nm = fmaxf(m, m2);
  if (nm > -INFINITY) {
    s = s * expf(m - nm) + s2 * expf(m2 - nm);
    m = nm;
  }
}

// sixteen logits (raw dot products in `a`, divided by T here) of query label lq against the rows gl + moco_vrow(v) < gend
template <bool LAB>
__device__ __forceinline__ void moco_ce_accum(const f32x16& a, float T, int gl, int gend, int64_t lq, const int64_t* __restrict__ qlab,
                                              float& m, float& s, float& ps, float& pc) {
  float x[16];
  float tm = -INFINITY;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    x[v] = gl + moco_vrow(v) < gend ? a[v] / T : -INFINITY;
    tm = fmaxf(tm, x[v]);
  }
  if (tm > -INFINITY) {
    const float nm = fmaxf(m, tm);
    float add = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) add += expf(x[v] - nm);       // a row past the slice: exp(-inf) = 0
    s = s * expf(m - nm) + add;
    m = nm;
  }
  if constexpr (LAB) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int g = gl + moco_vrow(v);
      if (g < gend && moco_is_pos(qlab[g], lq)) {
        ps += x[v];
        pc += 1.f;
      }
    }
  }
}

__device__ __forceinline__ void moco_store_logits(const f32x16& a, float T, int gl, int gend, float* __restrict__ orow /* out + q (K + 1) + 1 */) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int g = gl + moco_vrow(v);
    if (g < gend) orow[g] = a[v] / T;
  }
}

// rank, first sweep (BEST): the first of the lane's positive queue columns 1 + g in rank order
__device__ __forceinline__ void moco_best_accum(const f32x16& a, float T, int gl, int gend, int64_t lq, const int64_t* __restrict__ qlab,
                                                float& bv, int& bc) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int g = gl + moco_vrow(v);
    if (g < gend && moco_is_pos(qlab[g], lq)) {
      const float x = a[v] / T;
      if (moco_ahead(x, g + 1, bv, bc)) { bv = x; bc = g + 1; }
    }
  }
}

// rank, second sweep (COUNT): how many of the sixteen columns come before column tc with logit tv
__device__ __forceinline__ void moco_count_accum(const f32x16& a, float T, int gl, int gend, float tv, int tc, int& cnt) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int g = gl + moco_vrow(v);
    cnt += (g < gend && moco_ahead(a[v] / T, g + 1, tv, tc)) ? 1 : 0;
  }
}

__device__ __forceinline__ void moco_best_merge_halves(float& bv, int& bc) {
  const float v2 = __shfl_xor(bv, 32);
  const int c2 = __shfl_xor(bc, 32);
  if (moco_ahead(v2, c2, bv, bc)) { bv = v2; bc = c2; }
}

// both lane halves hold records of the same query: merge into both
__device__ __forceinline__ void moco_merge_halves(float& m, float& s, float& ps, float& pc) {
  const float m2 = __shfl_xor(m, 32), s2 = __shfl_xor(s, 32), ps2 = __shfl_xor(ps, 32), pc2 = __shfl_xor(pc, 32);
  const bool lo = (threadIdx.x & 32) == 0;                     // the same operand order in both halves: identical bits
  float ma = lo ? m : m2, sa = lo ? s : s2, mb = lo ? m2 : m, sb = lo ? s2 : s;
  moco_merge(ma, sa, mb, sb);
  m = ma; s = sa;
  ps = lo ? ps + ps2 : ps2 + ps;
  pc += pc2;
}

// ------------------------------------------------------------------------------------------
// the ring engine (forward)
// ------------------------------------------------------------------------------------------
template <int NK, int MODE, bool LAB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void moco_ring(
    const float* __restrict__ Q, int B, const float* __restrict__ Mem, int K, int D, float T, int per,
    float* __restrict__ out /* LOGITS: [B][K + 1] */, f32x4* __restrict__ part /* CE: [slices][B] (max, sum-exp, pos sum, pos count) */,
    const int64_t* __restrict__ klab, const int64_t* __restrict__ qlab,
    const MocoCol* __restrict__ thr /* COUNT: [B] the column to rank */, MocoCol* __restrict__ rpart /* BEST / COUNT: [slices][B] */) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(NK % 4 == 0, "a queue tile is a whole number of ring turns");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * 128;
  const int gbeg = blockIdx.y * per;
  const int gend = min(gbeg + per, K);
  const int q = q0 + 32 * wave + r;
  f32x4 qr[NK][4];
  slic_rt_load_frags(qr, Q + (int64_t)(q < B ? q : B - 1) * D, D, h);
  const SlicRtLane ln = slic_rt_lane(tid, D);
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(Mem + (int64_t)gbeg * D), 0, (int)((int64_t)(gend - gbeg) * D * 4), 0x00020000);    // rows past the slice: zeros
  unsigned goff[4];
  slic_rt_offsets(goff, ln, (unsigned)D * 4u);
  const int ntile = (gend - gbeg + MOCO_BG - 1) / MOCO_BG;
  auto issue = [&](int tile, int kt) {
    const bool live = ln.kin(kt) && tile < ntile;
    slic_rt_issue(rs_g, lds + (kt & 3) * SLIC_RT_TILE, wave, goff, (unsigned)tile * (unsigned)(MOCO_BG * D * 4), kt, live);
  };
  float m = -INFINITY, s = 0.f, ps = 0.f, pc = 0.f;
  int64_t lq = -1;
  if constexpr (LAB) lq = q < B ? klab[q] : -1;
  float* orow = nullptr;
  if constexpr (MODE == MOCO_LOGITS) orow = out + (int64_t)(q < B ? q : 0) * (K + 1) + 1;
  float bv = -INFINITY;                                        // BEST: the running best positive; COUNT: the column to rank
  int bc = INT_MAX, cnt = 0;
  if constexpr (MODE == MOCO_COUNT) {
    const MocoCol t = thr[q < B ? q : B - 1];
    bv = t.v; bc = t.c;
  }
  f32x16 acc[4];
  f32x4 a[2][4];
  slic_rt_ring_prime<4>(a, lds, r, h, [&](int kn) SLIC_RT_INLINE { issue(0, kn); });
  for (int tile = 0; tile < ntile; ++tile) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ct][v] = 0.f;
    // (the epilogue's stores and label loads may sit among the outstanding DMAs: they only make the counted wait stricter)
    auto step = [&](int kn) SLIC_RT_INLINE { issue(kn >= NK ? tile + 1 : tile, kn >= NK ? kn - NK : kn); };
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) slic_rt_ring_ktile<4, false, 4, false>(kt, acc, a, qr, lds, r, h, step, [](int) SLIC_RT_INLINE {});
    const int gl = gbeg + tile * MOCO_BG + 4 * h;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      if constexpr (MODE == MOCO_LOGITS) {
        if (q < B) moco_store_logits(acc[ct], T, gl + 32 * ct, gend, orow);
      } else if constexpr (MODE == MOCO_BEST) {
        moco_best_accum(acc[ct], T, gl + 32 * ct, gend, lq, qlab, bv, bc);
      } else if constexpr (MODE == MOCO_COUNT) {
        moco_count_accum(acc[ct], T, gl + 32 * ct, gend, bv, bc, cnt);
      } else {
        moco_ce_accum<LAB>(acc[ct], T, gl + 32 * ct, gend, lq, qlab, m, s, ps, pc);
      }
    }
  }
  if constexpr (MODE == MOCO_CE) {
    moco_merge_halves(m, s, ps, pc);
    if (h == 0 && q < B) {
      const f32x4 rec = {m, s, ps, pc};
      part[(int64_t)blockIdx.y * B + q] = rec;
    }
  }
  if constexpr (MODE == MOCO_BEST) {
    moco_best_merge_halves(bv, bc);
    if (h == 0 && q < B) rpart[(int64_t)blockIdx.y * B + q] = MocoCol{bv, bc};
  }
  if constexpr (MODE == MOCO_COUNT) {
    cnt += __shfl_xor(cnt, 32);
    if (h == 0 && q < B) rpart[(int64_t)blockIdx.y * B + q] = MocoCol{0.f, cnt};
  }
  slic_rt_wait<0>();                                           // the trailing all-zero DMAs must land before the workgroup leaves
}

// ------------------------------------------------------------------------------------------
// the 32-query engine (backward; forward of a D the DMA cannot address)
// ------------------------------------------------------------------------------------------
// columns c .. c + 3 of a row: zeros past D or when the row is not there.  VEC: D % 4 == 0 and 16-byte aligned rows
template <bool VEC>
__device__ __forceinline__ f32x4 moco_load4(const float* __restrict__ row, int c, int D, bool valid) {
  f32x4 z = {0.f, 0.f, 0.f, 0.f};
  if constexpr (VEC) return (valid && c < D) ? *(const f32x4*)(row + c) : z;
  else {
#pragma unroll
    for (int t = 0; t < 4; ++t) z[t] = (valid && c + t < D) ? row[c + t] : 0.f;
    return z;
  }
}

template <int NK, int MODE, bool LAB, bool VEC>
__global__ __launch_bounds__(256) void moco_tile32(
    const float* __restrict__ Q, int B, const float* __restrict__ Mem, int K, int D, float T, int per,
    float* __restrict__ out /* LOGITS: [B][K + 1] */, const float* __restrict__ dout /* LOGITS_BWD: [B][K + 1] */,
    f32x4* __restrict__ part /* CE */, const int64_t* __restrict__ klab, const int64_t* __restrict__ qlab,
    const float* __restrict__ lse, const float* __restrict__ npos /* CE_BWD: [B] each */,
    float* __restrict__ dqpart /* backward: [slices][B][D] */,
    const MocoCol* __restrict__ thr /* COUNT: [B] */, MocoCol* __restrict__ rpart /* BEST / COUNT: [slices][B] */) {
  constexpr bool BWD = MODE == MOCO_CE_BWD || MODE == MOCO_LOGITS_BWD;
  constexpr int NDT = NK / 4;                                  // d-tiles of 32 columns per wave: d-tile w + 4 i
  __shared__ float cs[BWD ? MOCO_BG * MOCO_CS_LD : 1];         // c[row of the tile][query]
  __shared__ f32x4 wst[MODE == MOCO_CE ? 4 * 32 : 1];
  __shared__ MocoCol rst[MODE == MOCO_BEST || MODE == MOCO_COUNT ? 4 * 32 : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.x * 32;
  const int q = q0 + r;
  const bool qv = q < B;
  const int gbeg = blockIdx.y * per;
  const int gend = min(gbeg + per, K);
  f32x4 qr[MODE == MOCO_LOGITS_BWD ? 1 : NK][4];
  if constexpr (MODE != MOCO_LOGITS_BWD) {
    const float* qrow = Q + (int64_t)(qv ? q : 0) * D;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt)
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) qr[kt][qd] = moco_load4<VEC>(qrow, 32 * kt + 8 * qd + 4 * h, D, qv);
  }
  float m = -INFINITY, s = 0.f, ps = 0.f, pc = 0.f;
  int64_t lq = -1;
  if constexpr (LAB) lq = qv ? klab[q] : -1;
  float lse_q = 0.f, wpos = 0.f;
  if constexpr (MODE == MOCO_CE_BWD) {
    lse_q = qv ? lse[q] : 0.f;
    wpos = qv ? 1.f / npos[q] : 0.f;
  }
  float* orow = nullptr;
  if constexpr (MODE == MOCO_LOGITS) orow = out + (int64_t)(qv ? q : 0) * (K + 1) + 1;
  float bv = -INFINITY;                                        // BEST: the running best positive; COUNT: the column to rank
  int bc = INT_MAX, cnt = 0;
  if constexpr (MODE == MOCO_COUNT) {
    const MocoCol t = thr[qv ? q : 0];
    bv = t.v; bc = t.c;
  }
  f32x16 dqacc[BWD ? NDT : 1];
  if constexpr (BWD) {
#pragma unroll
    for (int i = 0; i < NDT; ++i)
#pragma unroll
      for (int v = 0; v < 16; ++v) dqacc[i][v] = 0.f;
  }
  for (int g0 = gbeg; g0 < gend; g0 += MOCO_BG) {
    if constexpr (MODE != MOCO_LOGITS_BWD) {
      // this wave's 32 queue rows x the 32 queries; k order inside the accumulator: kt, qd, t ascending, lane half 0 then 1
      const int g = g0 + 32 * wave + r;
      const bool gv = g < gend;
      const float* mrow = Mem + (int64_t)(gv ? g : gend - 1) * D;
      f32x16 acc;
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
      for (int kt = 0; kt < NK; ++kt)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const f32x4 a4 = moco_load4<VEC>(mrow, 32 * kt + 8 * qd + 4 * h, D, gv);
#pragma unroll
          for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[t], qr[kt][qd][t], acc, 0, 0, 0);
        }
      const int gl = g0 + 32 * wave + 4 * h;                   // acc[v]: row gl + moco_vrow(v), query q
      if constexpr (MODE == MOCO_LOGITS) {
        if (qv) moco_store_logits(acc, T, gl, gend, orow);
      } else if constexpr (MODE == MOCO_CE) {
        moco_ce_accum<LAB>(acc, T, gl, gend, lq, qlab, m, s, ps, pc);
      } else if constexpr (MODE == MOCO_BEST) {
        moco_best_accum(acc, T, gl, gend, lq, qlab, bv, bc);
      } else if constexpr (MODE == MOCO_COUNT) {
        moco_count_accum(acc, T, gl, gend, bv, bc, cnt);
      } else {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int gg = gl + moco_vrow(v);
          float c = 0.f;
          if (qv && gg < gend) {
            c = expf(acc[v] / T - lse_q);
            if constexpr (LAB) c -= moco_is_pos(qlab[gg], lq) ? wpos : 0.f;
          }
          cs[(gg - g0) * MOCO_CS_LD + r] = c;
        }
      }
    } else {
      // the incoming gradient of the tile, transposed into cs: consecutive threads read consecutive columns of one dout row
      for (int e = tid; e < 32 * MOCO_BG; e += 256) {
        const int ql = e >> 7, gg = e & (MOCO_BG - 1);
        const bool ok = q0 + ql < B && g0 + gg < gend;
        cs[gg * MOCO_CS_LD + ql] = ok ? dout[(int64_t)(q0 + ql) * (K + 1) + 1 + g0 + gg] : 0.f;
      }
    }
    if constexpr (BWD) {
      __syncthreads();
      // dq^T[d, q] += sum over the tile's rows of memory[row, d] * c[row, q]; row order: pairs (2 step, 2 step + 1) ascending
#pragma unroll 8
      for (int step = 0; step < MOCO_BG / 2; ++step) {
        const int gg = 2 * step + h;
        const float b = cs[gg * MOCO_CS_LD + r];
        const bool gv = g0 + gg < gend;
        const float* mrow = Mem + (int64_t)(gv ? g0 + gg : gend - 1) * D;
#pragma unroll
        for (int i = 0; i < NDT; ++i) {
          const int d = (wave + 4 * i) * 32 + r;
          const float av = (gv && d < D) ? mrow[d] : 0.f;
          dqacc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, dqacc[i], 0, 0, 0);
        }
      }
      __syncthreads();                                         // cs is rewritten by the next tile
    }
  }
  if constexpr (MODE == MOCO_CE) {
    moco_merge_halves(m, s, ps, pc);
    if (h == 0) {
      const f32x4 rec = {m, s, ps, pc};
      wst[wave * 32 + r] = rec;
    }
    __syncthreads();
    if (wave == 0 && h == 0 && qv) {
      const f32x4 t = wst[r];
      float tm = t[0], ts = t[1], tp = t[2], tc = t[3];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const f32x4 u = wst[w * 32 + r];
        moco_merge(tm, ts, u[0], u[1]);
        tp += u[2];
        tc += u[3];
      }
      const f32x4 rec = {tm, ts, tp, tc};
      part[(int64_t)blockIdx.y * B + q] = rec;
    }
  }
  if constexpr (MODE == MOCO_BEST || MODE == MOCO_COUNT) {
    if constexpr (MODE == MOCO_BEST) moco_best_merge_halves(bv, bc);
    else cnt += __shfl_xor(cnt, 32);
    if (h == 0) rst[wave * 32 + r] = MODE == MOCO_BEST ? MocoCol{bv, bc} : MocoCol{0.f, cnt};
    __syncthreads();
    if (wave == 0 && h == 0 && qv) {
      MocoCol t = rst[r];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const MocoCol u = rst[w * 32 + r];
        if constexpr (MODE == MOCO_BEST) {
          if (moco_ahead(u.v, u.c, t.v, t.c)) t = u;
        } else {
          t.c += u.c;
        }
      }
      rpart[(int64_t)blockIdx.y * B + q] = t;
    }
  }
  if constexpr (BWD) {
    if (qv) {
      float* drow = dqpart + ((int64_t)blockIdx.y * B + q) * D;
#pragma unroll
      for (int i = 0; i < NDT; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int d = (wave + 4 * i) * 32 + 4 * h + moco_vrow(v);
          if (d < D) drow[d] = dqacc[i][v];
        }
    }
  }
}

// ------------------------------------------------------------------------------------------
// the positive column, the second stage of the forward, the reduction of the backward, the enqueue
// ------------------------------------------------------------------------------------------
// <a, b> by one wave: lane-strided partial sums, then a fixed xor tree; every lane returns the sum
__device__ __forceinline__ float moco_dot_wave(const float* __restrict__ a, const float* __restrict__ b, int D, int lane) {
  float x = 0.f;
  for (int d = lane; d < D; d += 64) x = fmaf(a[d], b[d], x);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

__global__ __launch_bounds__(256) void moco_pos_logit(const float* __restrict__ Q, const float* __restrict__ Kk, int B, int D, float T, int K,
                                                      float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float x = moco_dot_wave(Q + (int64_t)b * D, Kk + (int64_t)b * D, D, lane);
  if (lane == 0) out[(int64_t)b * (K + 1)] = x / T;
}

// stat [4][B]: l0 (the positive column's logit), lse, npos, rowloss.  One workgroup: a wave per query in turn, then the mean
__global__ __launch_bounds__(1024) void moco_ce_combine(const float* __restrict__ Q, const float* __restrict__ Kk, int B, int D, float T,
                                                        const f32x4* __restrict__ part, int S, float* __restrict__ stat,
                                                        float* __restrict__ loss) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += 16) {
    const float l0 = moco_dot_wave(Q + (int64_t)b * D, Kk + (int64_t)b * D, D, lane) / T;
    float m = -INFINITY, s = 0.f, ps = 0.f, pc = 0.f;
    for (int sl = lane; sl < S; sl += 64) {                    // the lane's slices ascending, then the tree: a fixed order
      const f32x4 u = part[(int64_t)sl * B + b];
      moco_merge(m, s, u[0], u[1]);
      ps += u[2];
      pc += u[3];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
      const bool lo = (lane & o) == 0;
      float ma = lo ? m : m2, sa = lo ? s : s2;
      moco_merge(ma, sa, lo ? m2 : m, lo ? s2 : s);
      m = ma; s = sa;
      const float p2 = __shfl_xor(ps, o);
      ps = lo ? ps + p2 : p2 + ps;
      pc += __shfl_xor(pc, o);
    }
    moco_merge(m, s, l0, 1.f);
    const float l = m + logf(s);
    const float np = pc + 1.f;
    if (lane == 0) {
      stat[b] = l0;
      stat[B + b] = l;
      stat[2 * B + b] = np;
      stat[3 * B + b] = l - (ps + l0) / np;
    }
  }
  __syncthreads();
  if (wave == 0) {
    float x = 0.f;
    for (int b = lane; b < B; b += 64) x += stat[3 * B + b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if (lane == 0) *loss = x / (float)B;
  }
}

// dq[b, d] = scale * (c0_b * k[b, d] + sum_s dqpart[s][b][d]), slices ascending.  CE: c0_b = exp(l0 - lse) - 1 / npos and
// scale = *gscale / (B T); else c0_b = dout[b, 0] and scale = 1 / T
template <bool CE>
__global__ __launch_bounds__(256) void moco_dq_reduce(const float* __restrict__ dqpart, int S, int B, int D, int K, float T,
                                                      const float* __restrict__ Kk, const float* __restrict__ stat,
                                                      const float* __restrict__ dout, const float* __restrict__ gscale,
                                                      float* __restrict__ dq) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)B * D) return;
  const int b = (int)(e / D);
  float c0, scale;
  if constexpr (CE) {
    c0 = expf(stat[b] - stat[B + b]) - 1.f / stat[2 * B + b];
    scale = (gscale ? *gscale : 1.f) / ((float)B * T);
  } else {
    c0 = dout[(int64_t)b * (K + 1)];
    scale = 1.f / T;
  }
  float x = c0 * Kk[e];
  for (int sl = 0; sl < S; ++sl) x += dqpart[(int64_t)sl * B * D + e];
  dq[e] = x * scale;
}

__global__ __launch_bounds__(256) void moco_enqueue(float* __restrict__ Mem, int64_t* __restrict__ qlab, const float* __restrict__ Kk,
                                                    const int64_t* __restrict__ klab, int B, int K, int D, int index) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)B * D) return;
  const int i = (int)(e / D), d = (int)(e % D);
  const int row = (index + i) % K;
  Mem[(int64_t)row * D + d] = Kk[e];
  if (d == 0 && qlab) qlab[row] = klab[i];
}

// ------------------------------------------------------------------------------------------
// rank of the best positive
// ------------------------------------------------------------------------------------------
struct MocoTopKs { int n, k[8]; };

// thr[b] = the first positive column of row b in rank order: column 0, or the best of the S per-slice records when it is strictly
// larger (an equal logit loses to column 0, the lower column).  One wave per query
__global__ __launch_bounds__(256) void moco_rank_thr(const float* __restrict__ Q, const float* __restrict__ Kk, int B, int D, float T,
                                                     const MocoCol* __restrict__ best, int S, MocoCol* __restrict__ thr) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float l0 = moco_dot_wave(Q + (int64_t)b * D, Kk + (int64_t)b * D, D, lane) / T;
  float bv = -INFINITY;
  int bc = INT_MAX;
  for (int sl = lane; sl < S; sl += 64) {
    const MocoCol u = best[(int64_t)sl * B + b];
    if (moco_ahead(u.v, u.c, bv, bc)) { bv = u.v; bc = u.c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o);
    const int c2 = __shfl_xor(bc, o);
    if (moco_ahead(v2, c2, bv, bc)) { bv = v2; bc = c2; }
  }
  if (lane == 0) thr[b] = moco_ahead(bv, bc, l0, 0) ? MocoCol{bv, bc} : MocoCol{l0, 0};
}

// hits[i] = the workgroup's sum of mine[i], i < ks.n: wave xor trees, then integer atomics in LDS.  Every thread of the workgroup calls it
__device__ __forceinline__ void moco_hits_reduce(const int (&mine)[8], const MocoTopKs& ks, int* __restrict__ hits) {
  __shared__ int sh[8];
  if (threadIdx.x < 8) sh[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int x = mine[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(&sh[i], x);
  }
  __syncthreads();
  if ((int)threadIdx.x < ks.n) hits[threadIdx.x] = sh[threadIdx.x];
}

// rank[b] = min(kmax, columns ahead: the S slice counts added), hits[i] = #{b : rank[b] < k_i}.  One workgroup; integer sums
__global__ __launch_bounds__(1024) void moco_rank_finish(const MocoCol* __restrict__ cnt, int S, int B, MocoTopKs ks, int* __restrict__ rank,
                                                         int* __restrict__ hits) {
  const int kmax = ks.k[ks.n - 1];
  int mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < B; b += 1024) {
    int c = 0;
    for (int sl = 0; sl < S; ++sl) c += cnt[(int64_t)sl * B + b].c;
    c = c < kmax ? c : kmax;
    if (rank) rank[b] = c;
#pragma unroll
    for (int i = 0; i < 8; ++i) mine[i] += (i < ks.n && c < ks.k[i]) ? 1 : 0;
  }
  moco_hits_reduce(mine, ks, hits);
}

// dense logits [B, C] and mask [B, C]: one wave per row, two passes.  best = the first masked column in rank order, rank = the columns
// ahead of it (C when the row has no masked column)
__global__ __launch_bounds__(256) void mask_rank_rows(const float* __restrict__ X, int ld, const unsigned char* __restrict__ Msk, int ldm,
                                                      int B, int C, int* __restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* x = X + (int64_t)b * ld;
  const unsigned char* mk = Msk + (int64_t)b * ldm;
  float bv = -INFINITY;
  int bc = INT_MAX;
  bool any = false;
  for (int c = lane; c < C; c += 64)
    if (mk[c]) {
      const float v = x[c];
      if (!any || moco_ahead(v, c, bv, bc)) { bv = v; bc = c; }
      any = true;
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o);
    const int c2 = __shfl_xor(bc, o);
    const bool a2 = __shfl_xor((int)any, o) != 0;
    if (a2 && (!any || moco_ahead(v2, c2, bv, bc))) { bv = v2; bc = c2; }
    any = any || a2;
  }
  int cnt = 0;
  for (int c = lane; c < C; c += 64) cnt += moco_ahead(x[c], c, bv, bc) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) rank[b] = any ? cnt : C;
}

// hits[i] = #{b : rank[b] < k_i}; one workgroup
__global__ __launch_bounds__(1024) void mask_rank_hits(const int* __restrict__ rank, int B, MocoTopKs ks, int* __restrict__ hits) {
  int mine[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < B; b += 1024) {
    const int c = rank[b];
#pragma unroll
    for (int i = 0; i < 8; ++i) mine[i] += (i < ks.n && c < ks.k[i]) ? 1 : 0;
  }
  moco_hits_reduce(mine, ks, hits);
}

// F.normalize(x, dim=1): y = x / max(||x||, eps), one wave per row; inv[b] = 1 / max(||x_b||, eps) is kept for the backward
__global__ __launch_bounds__(256) void moco_l2norm_fwd(const float* __restrict__ X, int B, int D, float eps, float* __restrict__ Y,
                                                       float* __restrict__ inv) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* x = X + (int64_t)b * D;
  const float n = sqrtf(moco_dot_wave(x, x, D, lane));
  const float s = 1.f / fmaxf(n, eps);
  for (int d = lane; d < D; d += 64) Y[(int64_t)b * D + d] = x[d] * s;
  if (lane == 0) inv[b] = n > eps ? s : -s;                    // the sign marks a clamped row: there y = x / eps is linear
}

// dx = inv (dy - y <dy, y>); a clamped row: dx = dy / eps
__global__ __launch_bounds__(256) void moco_l2norm_bwd(const float* __restrict__ dY, const float* __restrict__ Y, const float* __restrict__ inv,
                                                       int B, int D, float* __restrict__ dX) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* dy = dY + (int64_t)b * D;
  const float* y = Y + (int64_t)b * D;
  const float s = inv[b];
  const float t = s > 0.f ? moco_dot_wave(dy, y, D, lane) : 0.f;
  const float a = fabsf(s);
  for (int d = lane; d < D; d += 64) dX[(int64_t)b * D + d] = a * (dy[d] - y[d] * t);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// K-slices: about two rounds of workgroups over the device, at most `cap`; a slice is a whole number of tiles
static int moco_slices(int K, int qblocks, int cap, int* per_out) {
  const int tiles = (int)slic_cdiv(K, MOCO_BG);
  int cus = slic_device_cus();
  if (cus <= 0) cus = 256;
  int S = (int)slic_cdiv(2 * cus, qblocks);
  S = S > cap ? cap : S;
  S = S > tiles ? tiles : S;
  S = S < 1 ? 1 : S;
  const int per = (int)slic_cdiv(tiles, S) * MOCO_BG;
  *per_out = per;
  return (int)slic_cdiv(K, per);
}

static bool moco_vec_ok(const float* a, const float* b, int D) { return D % 4 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0; }

#define MOCO_NK_SWITCH(D, EXPR16, EXPR8, EXPR4) ((D) > 256 ? (EXPR16) : (D) > 128 ? (EXPR8) : (EXPR4))

// (spelled out: naming an instantiation to take its type would instantiate it, and BEST / COUNT exist for one value of LAB each)
using MocoRingFn = void (*)(const float*, int, const float*, int, int, float, int, float*, f32x4*, const int64_t*, const int64_t*,
                            const MocoCol*, MocoCol*);
using MocoTile32Fn = void (*)(const float*, int, const float*, int, int, float, int, float*, const float*, f32x4*, const int64_t*,
                              const int64_t*, const float*, const float*, float*, const MocoCol*, MocoCol*);

// forward of either mode: the ring where the DMA can address the rows, the 32-query engine otherwise
template <int MODE>
static int moco_forward(const float* q, const float* memory, int B, int K, int D, float T, float* out, f32x4* part, const int64_t* klab,
                        const int64_t* qlab, int* S_out, hipStream_t st, const MocoCol* thr = nullptr, MocoCol* rpart = nullptr) {
  const bool lab = klab != nullptr;
  if (moco_vec_ok(q, memory, D)) {
    int per;
    const int qb = (int)slic_cdiv(B, 128);
    const int S = moco_slices(K, qb, SLIC_MOCO_PARTS, &per);
    auto pick = [&](auto labc) {
      constexpr bool L = decltype(labc)::value;
      return MOCO_NK_SWITCH(D, (moco_ring<16, MODE, L>), (moco_ring<8, MODE, L>), (moco_ring<4, MODE, L>));
    };
    MocoRingFn kern;
    if constexpr (MODE == MOCO_BEST) kern = pick(std::true_type{});            // BEST runs with labels only, COUNT never reads them
    else if constexpr (MODE == MOCO_COUNT) kern = pick(std::false_type{});
    else kern = lab ? pick(std::true_type{}) : pick(std::false_type{});
    const size_t lds = (size_t)4 * SLIC_RT_TILE * sizeof(float);
    SLIC_LDS_LIMIT(kern, lds);
    kern<<<dim3((unsigned)qb, (unsigned)S), dim3(256), lds, st>>>(q, B, memory, K, D, T, per, out, part, klab, qlab, thr, rpart);
    SLIC_LAUNCH_CHECK();
    *S_out = S;
  } else {
    int per;
    const int qb = (int)slic_cdiv(B, 32);
    const int S = moco_slices(K, qb, SLIC_MOCO_PARTS, &per);
    auto pick = [&](auto labc) {
      constexpr bool L = decltype(labc)::value;
      return MOCO_NK_SWITCH(D, (moco_tile32<16, MODE, L, false>), (moco_tile32<8, MODE, L, false>), (moco_tile32<4, MODE, L, false>));
    };
    MocoTile32Fn kern;
    if constexpr (MODE == MOCO_BEST) kern = pick(std::true_type{});
    else if constexpr (MODE == MOCO_COUNT) kern = pick(std::false_type{});
    else kern = lab ? pick(std::true_type{}) : pick(std::false_type{});
    kern<<<dim3((unsigned)qb, (unsigned)S), dim3(256), 0, st>>>(q, B, memory, K, D, T, per, out, nullptr, part, klab, qlab, nullptr, nullptr, nullptr,
                                                               thr, rpart);
    SLIC_LAUNCH_CHECK();
    *S_out = S;
  }
  return SLIC_OK;
}

template <int MODE>
static int moco_backward(const float* q, const float* k, const float* memory, int B, int K, int D, float T, const float* dout,
                         const int64_t* klab, const int64_t* qlab, const float* stat, const float* gscale, float* dq, float* dqpart,
                         hipStream_t st) {
  const bool lab = klab != nullptr;
  const bool vec = moco_vec_ok(MODE == MOCO_CE_BWD ? q : memory, memory, D);
  int per;
  const int qb = (int)slic_cdiv(B, 32);
  const int S = moco_slices(K, qb, SLIC_MOCO_DQ_PARTS, &per);
#define MOCO_T32(NK) (lab ? (vec ? moco_tile32<NK, MODE, true, true> : moco_tile32<NK, MODE, true, false>) \
                          : (vec ? moco_tile32<NK, MODE, false, true> : moco_tile32<NK, MODE, false, false>))
  auto kern = MOCO_NK_SWITCH(D, MOCO_T32(16), MOCO_T32(8), MOCO_T32(4));
#undef MOCO_T32
  kern<<<dim3((unsigned)qb, (unsigned)S), dim3(256), 0, st>>>(q, B, memory, K, D, T, per, nullptr, dout, nullptr, klab, qlab,
                                                             stat ? stat + B : nullptr, stat ? stat + 2 * B : nullptr, dqpart, nullptr,
                                                             nullptr);
  SLIC_LAUNCH_CHECK();
  const unsigned nb = (unsigned)slic_cdiv((int64_t)B * D, 256);
  moco_dq_reduce<MODE == MOCO_CE_BWD><<<dim3(nb), dim3(256), 0, st>>>(dqpart, S, B, D, K, T, k, stat, dout, gscale, dq);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

#define MOCO_SHAPE_OK(B, K, D) ((B) > 0 && (K) > 0 && (D) > 0 && (D) <= 512 && (int64_t)(K) * (D) * 4 < (1ll << 31) && \
                                (int64_t)(B) * ((int64_t)(K) + 1) < (1ll << 40))

extern "C" int slic_moco_logits_fwd(const float* q, const float* k, const float* memory, int B, int K, int D, float T, float* out,
                                    void* stream) {
  SLIC_REQUIRE(q && k && memory && out, "slic_moco_logits_fwd: null pointer");
  SLIC_REQUIRE(MOCO_SHAPE_OK(B, K, D) && T > 0.f, "slic_moco_logits_fwd: need 1 <= D <= 512, K D < 2^29, T > 0 (B=%d K=%d D=%d)", B, K, D);
  int S;
  const int rc = moco_forward<MOCO_LOGITS>(q, memory, B, K, D, T, out, nullptr, nullptr, nullptr, &S, S_(stream));
  if (rc != SLIC_OK) return rc;
  moco_pos_logit<<<dim3((unsigned)slic_cdiv(B, 4)), dim3(256), 0, S_(stream)>>>(q, k, B, D, T, K, out);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_moco_logits_bwd(const float* dout, const float* k, const float* memory, int B, int K, int D, float T, float* dq,
                                    void* workspace, void* stream) {
  SLIC_REQUIRE(dout && k && memory && dq && workspace, "slic_moco_logits_bwd: null pointer");
  SLIC_REQUIRE(MOCO_SHAPE_OK(B, K, D) && T > 0.f, "slic_moco_logits_bwd: need 1 <= D <= 512, K D < 2^29, T > 0 (B=%d K=%d D=%d)", B, K, D);
  return moco_backward<MOCO_LOGITS_BWD>(nullptr, k, memory, B, K, D, T, dout, nullptr, nullptr, nullptr, nullptr, dq, (float*)workspace,
                                        S_(stream));
}

extern "C" int slic_moco_ce_fwd(const float* q, const float* k, const float* memory, int B, int K, int D, float T, const int64_t* k_label,
                                const int64_t* queue_label, float* stat, float* loss, void* workspace, void* stream) {
  SLIC_REQUIRE(q && k && memory && stat && loss && workspace, "slic_moco_ce_fwd: null pointer");
  SLIC_REQUIRE(MOCO_SHAPE_OK(B, K, D) && T > 0.f, "slic_moco_ce_fwd: need 1 <= D <= 512, K D < 2^29, T > 0 (B=%d K=%d D=%d)", B, K, D);
  SLIC_REQUIRE((k_label == nullptr) == (queue_label == nullptr), "slic_moco_ce_fwd: k_label and queue_label come together");
  SLIC_REQUIRE(((uintptr_t)workspace % 16) == 0, "slic_moco_ce_fwd: unaligned workspace");
  int S;
  const int rc = moco_forward<MOCO_CE>(q, memory, B, K, D, T, nullptr, (f32x4*)workspace, k_label, queue_label, &S, S_(stream));
  if (rc != SLIC_OK) return rc;
  moco_ce_combine<<<dim3(1), dim3(1024), 0, S_(stream)>>>(q, k, B, D, T, (const f32x4*)workspace, S, stat, loss);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_moco_ce_bwd(const float* q, const float* k, const float* memory, int B, int K, int D, float T, const int64_t* k_label,
                                const int64_t* queue_label, const float* stat, const float* gscale, float* dq, void* workspace,
                                void* stream) {
  SLIC_REQUIRE(q && k && memory && stat && dq && workspace, "slic_moco_ce_bwd: null pointer");
  SLIC_REQUIRE(MOCO_SHAPE_OK(B, K, D) && T > 0.f, "slic_moco_ce_bwd: need 1 <= D <= 512, K D < 2^29, T > 0 (B=%d K=%d D=%d)", B, K, D);
  SLIC_REQUIRE((k_label == nullptr) == (queue_label == nullptr), "slic_moco_ce_bwd: k_label and queue_label come together");
  return moco_backward<MOCO_CE_BWD>(q, k, memory, B, K, D, T, nullptr, k_label, queue_label, stat, gscale, dq, (float*)workspace,
                                    S_(stream));
}

extern "C" int slic_moco_enqueue(float* memory, int64_t* queue_label, const float* k, const int64_t* k_label, int B, int K, int D, int index,
                                 void* stream) {
  SLIC_REQUIRE(memory && k, "slic_moco_enqueue: null pointer");
  SLIC_REQUIRE(B > 0 && D > 0 && B <= K && index >= 0 && index < K, "slic_moco_enqueue: need 0 < B <= K, 0 <= index < K (B=%d K=%d index=%d)",
               B, K, index);
  SLIC_REQUIRE(!queue_label || k_label, "slic_moco_enqueue: queue_label without k_label");
  moco_enqueue<<<dim3((unsigned)slic_cdiv((int64_t)B * D, 256)), dim3(256), 0, S_(stream)>>>(memory, queue_label, k, k_label, B, K, D, index);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

static bool moco_topks_ok(const int32_t* top_ks, int n_ks, int64_t kcap, MocoTopKs* ks) {
  if (!top_ks || n_ks < 1 || n_ks > 8) return false;
  ks->n = n_ks;
  for (int i = 0; i < 8; ++i) ks->k[i] = 0;
  for (int i = 0; i < n_ks; ++i) {
    if (top_ks[i] < 1 || top_ks[i] > kcap || (i > 0 && top_ks[i] <= top_ks[i - 1])) return false;
    ks->k[i] = top_ks[i];
  }
  return true;
}

extern "C" int slic_moco_topk_hits(const float* q, const float* k, const float* memory, int B, int K, int D, float T, const int64_t* k_label,
                                   const int64_t* queue_label, const int32_t* top_ks, int n_ks, int32_t* rank, int32_t* hits,
                                   void* workspace, void* stream) {
  SLIC_REQUIRE(q && k && memory && hits && workspace, "slic_moco_topk_hits: null pointer");
  SLIC_REQUIRE(MOCO_SHAPE_OK(B, K, D) && T > 0.f, "slic_moco_topk_hits: need 1 <= D <= 512, K D < 2^29, T > 0 (B=%d K=%d D=%d)", B, K, D);
  SLIC_REQUIRE((k_label == nullptr) == (queue_label == nullptr), "slic_moco_topk_hits: k_label and queue_label come together");
  SLIC_REQUIRE(((uintptr_t)workspace % 8) == 0, "slic_moco_topk_hits: unaligned workspace");
  MocoTopKs ks;
  SLIC_REQUIRE(moco_topks_ok(top_ks, n_ks, 8, &ks), "slic_moco_topk_hits: top_ks: 1 .. 8 ascending values in 1 .. 8 (n_ks=%d)", n_ks);
  MocoCol* thr = (MocoCol*)workspace;                          // [B], then [SLIC_MOCO_PARTS][B] slice records
  MocoCol* rpart = thr + B;
  int S = 0;
  if (k_label) {                                               // first sweep: the best positive of the queue
    const int rc = moco_forward<MOCO_BEST>(q, memory, B, K, D, T, nullptr, nullptr, k_label, queue_label, &S, S_(stream), nullptr, rpart);
    if (rc != SLIC_OK) return rc;
  }
  moco_rank_thr<<<dim3((unsigned)slic_cdiv(B, 4)), dim3(256), 0, S_(stream)>>>(q, k, B, D, T, rpart, S, thr);
  SLIC_LAUNCH_CHECK();
  const int rc = moco_forward<MOCO_COUNT>(q, memory, B, K, D, T, nullptr, nullptr, nullptr, nullptr, &S, S_(stream), thr, rpart);
  if (rc != SLIC_OK) return rc;
  moco_rank_finish<<<dim3(1), dim3(1024), 0, S_(stream)>>>(rpart, S, B, ks, rank, hits);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_mask_topk_hits(const float* logits, int ld, const uint8_t* mask, int ldm, int B, int C, const int32_t* top_ks, int n_ks,
                                   int32_t* rank, int32_t* hits, void* stream) {
  SLIC_REQUIRE(logits && mask && rank && hits, "slic_mask_topk_hits: null pointer");
  SLIC_REQUIRE(B > 0 && C > 0 && ld >= C && ldm >= C, "slic_mask_topk_hits: need B, C > 0 and ld, ldm >= C (B=%d C=%d ld=%d ldm=%d)", B, C,
               ld, ldm);
  MocoTopKs ks;
  SLIC_REQUIRE(moco_topks_ok(top_ks, n_ks, C, &ks), "slic_mask_topk_hits: top_ks: 1 .. 8 ascending values in 1 .. C (n_ks=%d)", n_ks);
  mask_rank_rows<<<dim3((unsigned)slic_cdiv(B, 4)), dim3(256), 0, S_(stream)>>>(logits, ld, mask, ldm, B, C, rank);
  SLIC_LAUNCH_CHECK();
  mask_rank_hits<<<dim3(1), dim3(1024), 0, S_(stream)>>>(rank, B, ks, hits);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_l2normalize_fwd(const float* x, int B, int D, float eps, float* y, float* inv, void* stream) {
  SLIC_REQUIRE(x && y && inv, "slic_l2normalize_fwd: null pointer");
  SLIC_REQUIRE(B > 0 && D > 0 && eps > 0.f, "slic_l2normalize_fwd: need B, D, eps > 0 (B=%d D=%d)", B, D);
  moco_l2norm_fwd<<<dim3((unsigned)slic_cdiv(B, 4)), dim3(256), 0, S_(stream)>>>(x, B, D, eps, y, inv);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_l2normalize_bwd(const float* dy, const float* y, const float* inv, int B, int D, float* dx, void* stream) {
  SLIC_REQUIRE(dy && y && inv && dx, "slic_l2normalize_bwd: null pointer");
  SLIC_REQUIRE(B > 0 && D > 0, "slic_l2normalize_bwd: need B, D > 0 (B=%d D=%d)", B, D);
  moco_l2norm_bwd<<<dim3((unsigned)slic_cdiv(B, 4)), dim3(256), 0, S_(stream)>>>(dy, y, inv, B, D, dx);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
