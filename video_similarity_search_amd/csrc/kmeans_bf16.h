// Certified bf16 E-step of k-means (slic_kmeans_assign_bf16, slic_kmeans_lloyd_step_bf16, slic_kmeans_lloyd_local_bf16): part of
// kmeans.hip, which includes this file after its own kernels and launch helpers (km_block_hist, km_accumulate_impl, KmFinish).
//
// The score GEMM runs on v_mfma_f32_32x32x16_bf16 over round-to-nearest-even images of the rows and only NOMINATES centroids:
//   1. km_assign_bf16: coarse scores cs = fmaf(-2, acc, cnorm[j]) of a 128-centroid block against the streamed points, the per-pair
//      bound b(i, j) (|cs - s| <= b for the exact score s), the block's ub = min_j (cs + b), and the centroids with
//      cs - b <= ub as (index, cs - b) pairs in KMB_CAP slots per (row, block), at fixed positions;
//   2. km_bf16_combine: ub_i = min over the blocks; a row with ONE pair left under ub_i and no overflowed block has its label; every
//      other row goes on a list (a block that overflowed its slots counts only if its smallest cs - b passes ub_i);
//   3. km_bf16_rescore: one wave per listed row, one lane per surviving pair: the exact chain acc = fmaf(x[k], c[k], acc), k ascending
//      from +0, score fmaf(-2, acc, cnorm[j]) — the bits km_assign_creg's MFMA chain produces — and the argmin by (score, lower index).
//      A row with an overflowed block (or with no pair at all: a NaN row) runs the chain over ALL K centroids instead.
// The true argmin j* is always a pair: cs(j*) - b(j*) <= s(j*) <= s(j') <= cs(j') + b(j') for every j', and a minimum over a subset of
// the centroids (a block) is >= ub_i, so filtering by it only keeps more.  So is every centroid that ties with j* in s.  The bf16 scores
// never reach an output: the labels are the fp32 kernels' labels, bit for bit.
// Integer atomics only (the list length, the statistics, n_changed, the histogram): exact in any order.  Every loop has a
// bound known at launch.
#pragma once
#include "bf16_image.h"

#define KMB_CAP 8             // (index, cs - b) slots per (row, 128-centroid block)

// One workgroup: 4 waves x 32 centroids in registers (NK x 16 registers per lane: k-tiles of 64 bf16 columns; 4: D <= 256, 8: D <= 512),
// the points of its slice streaming through the 4-stage ring of mfma_ring.h read as bytes (128 rows x 128 bytes per stage), one
// ds_read_b128 per MFMA: the structural twin of km_assign_creg and topk_collect_bf16.  Grid: slices x 128-centroid blocks.
// Accumulator element g of lane (r, h) is centroid cbase + (g & 3) + 8 (g >> 2) + 4 h against point 32 pt + r.
template <int NK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void km_assign_bf16(
    const float* __restrict__ Xb, const float* __restrict__ xnorm, int64_t N, int Df, int D, const float* __restrict__ Cb, int K,
    const float* __restrict__ cnorm, float* __restrict__ pub /* [ncb][N] */, int32_t* __restrict__ pcnt /* [ncb][N] */,
    float* __restrict__ plo /* [ncb][N]: the block's min (cs - b), written where the block overflowed */,
    unsigned long long* __restrict__ cand /* [ncb][KMB_CAP][N]: {centroid, bits of cs - b} */, int32_t* z0, int32_t* z1, int32_t* z2) {
  extern __shared__ __attribute__((aligned(16))) float km_lds[];
  static_assert(NK % 4 == 0, "a point tile is a whole number of ring turns");
  // the iteration's device counters (labels changed; M-step workgroups done; rows listed for the rescore) start at zero: nothing before
  // this kernel in the iteration touches them, everything after it is ordered behind it on the stream
  if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
    if (z0) *z0 = 0;
    if (z1) *z1 = 0;
    if (z2) *z2 = 0;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  // this workgroup's points: km_assign_creg's even split of the 32-point sub-tiles over the slices, walked as 128-point tiles
  const int64_t subs = (N + 31) / 32;
  const int64_t u0 = subs * blockIdx.x / gridDim.x, u1 = subs * (blockIdx.x + 1) / gridDim.x;
  const int ntile = (int)((u1 - u0 + 3) / 4);
  const int64_t pbeg = u0 * 32;
  const int64_t prow = (N - pbeg) < (u1 - u0) * 32 ? (N - pbeg) : (u1 - u0) * 32;               // rows of the slice
  const int64_t pend = pbeg + prow;
  const int cbase = (blockIdx.y * 4 + wave) * 32;
  f32x4 cr[NK][4];
  {
    const int crow = cbase + r;
    slic_rt_load_frags(cr, Cb + (int64_t)(crow < K ? crow : K - 1) * Df, Df, h, crow < K);
  }
  // b(i, j) = ||x_i|| cb[g] + cc[g]  (§7f: 2 eps ||x|| ||c|| + 2^-22 (cnorm + 2 ||x|| ||c||) + the subnormal terms)
  float cn[16], cb[16], cc[16];
  unsigned kmask = 0u;
  const float absu = (float)D * 0x1p-125f;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int c = cbase + (g & 3) + 8 * (g >> 2) + 4 * h;
    const bool v = c < K;
    const float q = cnorm[v ? c : K - 1];                     // (unconditional: the sixteen loads go out together)
    const float nc = sqrtf(q);
    cn[g] = v ? q : INFINITY;
    cb[g] = v ? fmaf(nc, 2.f * TK_BF16_EPS + 0x1p-21f, absu) : 0.f;
    cc[g] = v ? fmaf(q, 0x1p-22f, absu * (1.f + nc)) : 0.f;
    kmask |= v ? (1u << g) : 0u;
  }
  const SlicRtLane ln = slic_rt_lane(tid, Df);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)(Xb + pbeg * (int64_t)Df), 0, (int)(prow * (int64_t)Df * 4),
                                                                        0x00020000);            // rows past the slice: zeros
  unsigned xoff[4];
  slic_rt_offsets(xoff, ln, (unsigned)Df * 4u);
  auto issue = [&](int tile, int kt) SLIC_RT_INLINE {
    const bool live = ln.kin(kt) && tile < ntile;
    slic_rt_issue(rs_x, km_lds + (kt & 3) * SLIC_RT_TILE, wave, xoff, (unsigned)tile * (unsigned)(128 * Df * 4), kt, live);
  };
  float* xch = km_lds + 4 * SLIC_RT_TILE;                      // [wave 4][point 128]: the waves' min (cs + b) of the finished tile
  int* wcnt = (int*)(xch + 4 * 128);                           // [wave 4][point 128]: the waves' pairs of the tile's rows
  float* xlo = xch + 8 * 128;                                  // [wave 4][point 128]: the waves' min (cs - b)
  const int64_t blkN = (int64_t)blockIdx.y * N;
  f32x16 acc[4];
  f32x4 a[2][4];
  slic_rt_ring_prime<4>(a, km_lds, r, h, [&](int kn) SLIC_RT_INLINE { issue(0, kn); });
  for (int tile = 0; tile < ntile; ++tile) {
    const int64_t p0 = pbeg + (int64_t)tile * 128;
    float nx[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int64_t p = p0 + 32 * pt + r;
      nx[pt] = p < pend ? xnorm[p] : 0.f;
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[pt][v] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
      // ring step s = (tile, kt), the contract of slic_rt_ring_ktile: step s + 1 has landed, the barrier publishes it and frees the
      // stage of step s - 1 for the DMAs of step s + 3
      slic_rt_wait<4>();
      __builtin_amdgcn_s_barrier();
      issue(kt + 3 >= NK ? tile + 1 : tile, kt + 3 >= NK ? kt + 3 - NK : kt + 3);
      const float* Ts = km_lds + (kt & 3) * SLIC_RT_TILE;
      const float* Tn = km_lds + ((kt + 1) & 3) * SLIC_RT_TILE;
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        const int cur = qd & 1, nxt = cur ^ 1;
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
          a[nxt][pt] = qd < 3 ? *(const f32x4*)&Ts[slic_rt_off(32 * pt + r, 2 * (qd + 1) + h)]
                              : *(const f32x4*)&Tn[slic_rt_off(32 * pt + r, h)];       // first fragments of the next step
#pragma unroll
        for (int pt = 0; pt < 4; ++pt)
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(tkb_bf16x8, cr[kt][qd]),
                                                            __builtin_bit_cast(tkb_bf16x8, a[cur][pt]), acc[pt], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    // ---- the tile's epilogue.  acc becomes cs - b; the wave's min (cs + b) per point goes to the other waves through LDS
    float lmin[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      float m = INFINITY, lm = INFINITY;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float cs = __builtin_fmaf(-2.0f, acc[pt][g], cn[g]);
        const float b = __builtin_fmaf(nx[pt], cb[g], cc[g]);
        const float hi = cs + b, lo = cs - b;
        acc[pt][g] = lo;
        m = hi < m ? hi : m;                                   // (a NaN never lowers it; a centroid past K has cs = +inf)
        lm = lo < lm ? lo : lm;
      }
      const float om = __shfl_xor(m, 32);
      m = om < m ? om : m;
      lmin[pt] = lm;
      if (h == 0) xch[wave * 128 + 32 * pt + r] = m;
    }
    // this wave's ds_writes must have reached LDS before the barrier publishes them (gfx950's barrier does not imply it); only LGKM is
    // waited for: the ring's DMAs stay in flight
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // the block's ub per point; this lane's pairs under it, the lane pair's, the wave's -> LDS.  Slots are FIXED positions: waves
    // ascending, lane half 0 then 1, g ascending (no atomics; the same image on every run)
    float ubv[4];
    int nl[4], off[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int64_t p = p0 + 32 * pt + r;
      float ub = xch[32 * pt + r];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float o = xch[w * 128 + 32 * pt + r];
        ub = o < ub ? o : ub;
      }
      ubv[pt] = ub;
      int n = 0;
      if (p < pend && lmin[pt] <= ub) {
#pragma unroll
        for (int g = 0; g < 16; ++g) n += (((kmask >> g) & 1u) && acc[pt][g] <= ub) ? 1 : 0;
      }
      const int no = __shfl_xor(n, 32);
      nl[pt] = n;
      off[pt] = h ? no : 0;
      const float olm = __shfl_xor(lmin[pt], 32);
      if (h == 0) {
        wcnt[wave * 128 + 32 * pt + r] = n + no;
        xlo[wave * 128 + 32 * pt + r] = olm < lmin[pt] ? olm : lmin[pt];
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int64_t p = p0 + 32 * pt + r;
      int base = off[pt], total = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int c = wcnt[w * 128 + 32 * pt + r];
        base += w < wave ? c : 0;
        total += c;
      }
      if (p < pend) {
        if (wave == pt && h == 0) {
          pub[blkN + p] = ubv[pt];
          pcnt[blkN + p] = total;                              // > KMB_CAP: the block overflowed for this row ...
          if (total > KMB_CAP) {                               // ... which matters only if its smallest cs - b can pass ub_i (km_bf16_combine)
            float blo = xlo[32 * pt + r];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
              const float o = xlo[w * 128 + 32 * pt + r];
              blo = o < blo ? o : blo;
            }
            plo[blkN + p] = blo;
          }
        }
        if (nl[pt] > 0) {
          int slot = base;
#pragma unroll
          for (int g = 0; g < 16; ++g)
            if (((kmask >> g) & 1u) && acc[pt][g] <= ubv[pt]) {
              if (slot >= 0 && slot < KMB_CAP)                 // every slot write is guarded against the cap
                cand[((int64_t)blockIdx.y * KMB_CAP + slot) * N + p] =
                    ((unsigned long long)(unsigned)(cbase + (g & 3) + 8 * (g >> 2) + 4 * h) << 32) | __float_as_uint(acc[pt][g]);
              ++slot;
            }
        }
      }
    }
  }
  slic_rt_wait<0>();                                           // the trailing all-zero DMAs must land before the workgroup leaves
}

// ||x_i|| of every row (one wave per row; any summation order: the bound has room for its error, §7f)
__global__ __launch_bounds__(256) void km_bf16_rownorm(const float* __restrict__ X, int64_t N, int D, int64_t ldx, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;
  float s = 0.f;
  for (int k = lane * 4; k < D; k += 256) {
    const f32x4 v = *(const f32x4*)(X + i * ldx + k);
    s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) out[i] = sqrtf(s);
}

// One thread per row: ub_i over the blocks, the pairs left under it.  One pair and no block that lost a pair under ub_i: the label, with the side
// products of km_combine (n_changed, HIST: the per-1024-row label histogram bc — of the rows decided HERE; km_bf16_rescore adds its rows).
// Every other row: on the list, bit 31 set when the exact pass must run over all K centroids.
// stats += {rows listed, rows for the all-K pass, pairs of all rows (K for an all-K row)}.
template <bool HIST>
__global__ void km_bf16_combine(const float* __restrict__ pub, const int32_t* __restrict__ pcnt, const float* __restrict__ plo,
                                const unsigned long long* __restrict__ cand,
                                int G, int64_t N, int K, int32_t* __restrict__ labels, const int32_t* __restrict__ labels_old,
                                int32_t* n_changed, int32_t* __restrict__ bc, float* __restrict__ rowub, uint32_t* __restrict__ list,
                                int32_t* nlist, int32_t* __restrict__ stats) {
  extern __shared__ int km_hist_b[];
  __shared__ int bst[4];                                       // the workgroup's {changed, listed, all-K, pairs}: one global atomic each
  if (threadIdx.x < 4) bst[threadIdx.x] = 0;
  if constexpr (!HIST) __syncthreads();
  if constexpr (HIST) {
    for (int j = threadIdx.x; j < K; j += blockDim.x) km_hist_b[j] = 0;
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int changed = 0, listed = 0, allk = 0, ns = 0;
  if (i < N) {
    float ub = INFINITY;
    for (int g = 0; g < G; ++g) {
      const float u = pub[(int64_t)g * N + i];
      ub = u < ub ? u : ub;
    }
    // a block with more pairs under ITS ub than slots lost some; none of them matters unless the block's smallest cs - b passes ub_i
    // (!(x > ub): a NaN counts as passing)
    bool over = false;
    int first = 0;
    for (int g = 0; g < G; ++g) {
      const int c = pcnt[(int64_t)g * N + i];
      if (c > KMB_CAP) {
        over |= !(plo[(int64_t)g * N + i] > ub);
        continue;
      }
      for (int s = 0; s < c; ++s) {
        const unsigned long long e = cand[((int64_t)g * KMB_CAP + s) * N + i];
        if (__uint_as_float((unsigned)e) <= ub) { first = (int)(e >> 32); ++ns; }
      }
    }
    if (!over && ns == 1) {
      labels[i] = first;
      if (labels_old) changed = labels_old[i] != first;
      if constexpr (HIST) atomicAdd(&km_hist_b[first], 1);
    } else {
      listed = 1;
      allk = (over || ns == 0) ? 1 : 0;
      if (allk) ns = K;
      rowub[i] = ub;
    }
  }
  {
    const unsigned long long mc = __ballot(changed), ml = __ballot(listed), ma = __ballot(allk);
    // the list grows by one atomic per wave: lane 0 reserves the wave's entries, every listed lane takes the next one in lane order
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && ml) base = atomicAdd(nlist, (int)__popcll(ml));
    base = __shfl(base, 0);
    if (listed) list[base + (int)__popcll(ml & ((1ull << lane) - 1ull))] = (uint32_t)i | (allk ? 0x80000000u : 0u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ns += __shfl_xor(ns, o);
    if (lane == 0) {
      if (mc) atomicAdd(&bst[0], (int)__popcll(mc));
      if (ml) atomicAdd(&bst[1], (int)__popcll(ml));
      if (ma) atomicAdd(&bst[2], (int)__popcll(ma));
      if (ns) atomicAdd(&bst[3], ns);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (labels_old && bst[0]) atomicAdd(n_changed, bst[0]);
    if (stats) {
      if (bst[1]) atomicAdd(stats, bst[1]);
      if (bst[2]) atomicAdd(stats + 1, bst[2]);
      if (bst[3]) atomicAdd(stats + 2, bst[3]);
    }
  }
  if constexpr (HIST) {
    for (int j = threadIdx.x; j < K; j += blockDim.x) bc[(int64_t)blockIdx.x * K + j] = km_hist_b[j];
  }
}

// One wave per listed row, the waves striding over the list (its length is on the device; the trip count is bounded by N).  A lane
// takes one pair (or, all-K rows, the centroids lane, lane + 64, ..): the exact chain from the fp32 rows in natural column order,
// k ascending from +0 — X and C here are NOT the k8-permuted copies — and the score fmaf(-2, acc, cnorm[j]); then the argmin by
// (score, lower index), a NaN never winning and a row without a finite-or-inf winner taking label 0, as km_combine decides it.
__global__ __launch_bounds__(256) void km_bf16_rescore(const float* __restrict__ X, int64_t N, int D, int64_t ldx, const float* __restrict__ C,
                                                       int K, int64_t ldc, const float* __restrict__ cnorm, int G,
                                                       const int32_t* __restrict__ pcnt, const unsigned long long* __restrict__ cand,
                                                       const float* __restrict__ rowub, const uint32_t* __restrict__ list,
                                                       const int32_t* __restrict__ nlist, int32_t* __restrict__ labels,
                                                       const int32_t* __restrict__ labels_old, int32_t* n_changed, int32_t* __restrict__ bc) {
  __shared__ __attribute__((aligned(16))) float xs_all[4][512];     // a wave's row (D <= 512), read back as broadcasts
  const int lane = threadIdx.x & 63;
  float* xs = xs_all[threadIdx.x >> 6];
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t nl = *nlist;
  nl = nl < N ? nl : N;
  for (int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < nl; e += nw) {
    const uint32_t raw = __builtin_amdgcn_readfirstlane(list[e]);
    const int64_t i = raw & 0x7FFFFFFFu;
    const bool allk = raw >> 31;
    if (i >= N) continue;                                      // (never: the list holds row ids)
    // the row goes to LDS once, coalesced (through the scalar cache its 2 KB per row queued behind each other: 144 us per E-step at
    // 100k x 512, a sixth of the rows listed).  Same wave, LDS operations in order: the fences only keep the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int k = lane * 4; k < D; k += 256) *(f32x4*)(xs + k) = *(const f32x4*)(X + i * ldx + k);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const float ub = rowub[i];
    const int np = allk ? K : G * KMB_CAP;
    float best = INFINITY;
    int bidx = 0x7fffffff;
    for (int p0 = 0; p0 < np; p0 += 64) {
      const int p = p0 + lane;
      int j = -1;
      if (p < np) {
        if (allk) j = p;
        else {
          const int g = p / KMB_CAP, s = p - g * KMB_CAP;
          const int c = pcnt[(int64_t)g * N + i];             // (> KMB_CAP: a block whose pairs are all above ub_i on these rows)
          if (c <= KMB_CAP && s < c) {
            const unsigned long long cd = cand[((int64_t)g * KMB_CAP + s) * N + i];
            if (__uint_as_float((unsigned)cd) <= ub) j = (int)(cd >> 32);
          }
        }
      }
      const bool live = j >= 0 && j < K;
      if (!__any(live)) continue;                              // (wave-uniform)
      // the k loop's trip count is uniform; only the lanes with a pair load and compute (an idle lane's sixteen loads per batch would
      // be 2 KB of L2 traffic per lane and row for nothing).  The loads of a 64-column batch go out together; the chain itself stays one
      // accumulator, k ascending
      const float* c = C + (int64_t)(live ? j : 0) * ldc;
      float acc = 0.f;
      for (int k0 = 0; k0 < D; k0 += 64) {
        f32x4 cv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int k = k0 + 4 * u;
          const f32x4 z = {0.f, 0.f, 0.f, 0.f};
          cv[u] = live ? *(const f32x4*)(c + (k < D ? k : 0)) : z;        // D % 8 == 0: a 4-column chunk is inside the row or past it
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int k = k0 + 4 * u;
          if (k < D) {                                         // (uniform)
            const f32x4 xv = *(const f32x4*)(xs + k);
            acc = fmaf(xv.x, cv[u].x, acc); acc = fmaf(xv.y, cv[u].y, acc); acc = fmaf(xv.z, cv[u].z, acc); acc = fmaf(xv.w, cv[u].w, acc);
          }
        }
      }
      if (live) {
        const float sc = fmaf(-2.0f, acc, cnorm[j]);
        if (sc < best || (sc == best && j < bidx)) { best = sc; bidx = j; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bidx, o);
      if (ob < best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if (lane == 0) {
      const int idx = (bidx < 0 || bidx >= K) ? 0 : bidx;
      labels[i] = idx;
      if (labels_old && labels_old[i] != idx) atomicAdd(n_changed, 1);
      if (bc) atomicAdd(&bc[(i / KM_SB) * K + idx], 1);
    }
  }
}

// ------------------------------------ C ABI ------------------------------------------------

static bool km_bf16_domain(int64_t N, int K, int D) { return N > 0 && N < (1ll << 31) && K > 0 && D > 0 && D % 8 == 0 && D <= 512; }
static int km_bf16_dp(int D) { return (D + 15) / 16 * 16; }

extern "C" float slic_kmeans_bf16_eps(void) { return TK_BF16_EPS; }

extern "C" int slic_kmeans_bf16_plan(int64_t N, int K, int D, int64_t* out) {
  SLIC_REQUIRE(out && N > 0 && K > 0 && D > 0, "slic_kmeans_bf16_plan: bad args");
  const bool on = km_bf16_domain(N, K, D);
  const int Dp = km_bf16_dp(D);
  out[0] = on ? 1 : 0; out[1] = on ? Dp : 0; out[2] = on ? KMB_CAP : 0; out[3] = on ? slic_cdiv(K, 128) : 0;
  out[4] = on ? N * Dp * 2 : 0; out[5] = on ? (int64_t)K * Dp * 2 : 0;
  return SLIC_OK;
}

extern "C" int slic_kmeans_bf16_image(const float* X, int64_t N, int D, int ldx, void* image, float* norms, void* stream) {
  SLIC_REQUIRE(X && image && N > 0, "slic_kmeans_bf16_image: null pointer");
  SLIC_REQUIRE(D > 0 && D % 8 == 0 && D <= 512 && ldx % 4 == 0 && ldx >= D, "slic_kmeans_bf16_image: need D %% 8 == 0, D <= 512 and 16-byte aligned rows (D=%d ldx=%d)", D, ldx);
  SLIC_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)image % 16) == 0, "slic_kmeans_bf16_image: unaligned");
  const int Dp = km_bf16_dp(D);
  tkb_convert<<<dim3((unsigned)slic_cdiv(N * (Dp / 8), 256)), dim3(256), 0, S_(stream)>>>(X, N, D, ldx, Dp, (uint4*)image);
  SLIC_LAUNCH_CHECK();
  if (norms) {
    km_bf16_rownorm<<<dim3((unsigned)slic_cdiv(N, 4)), dim3(256), 0, S_(stream)>>>(X, N, D, ldx, norms);
    SLIC_LAUNCH_CHECK();
  }
  return SLIC_OK;
}

extern "C" size_t slic_kmeans_assign_bf16_workspace_bytes(int64_t N, int K) {
  const size_t ncb = (size_t)slic_cdiv(K, 128);
  return 3 * slic_align_up(ncb * N * 4, 256) + slic_align_up(ncb * KMB_CAP * N * 8, 256) + 2 * slic_align_up((size_t)N * 4, 256) + 256;
}

// bc (optional): also the M-step's per-1024-row-block label histogram; z0 / z1: the iteration counters km_assign_creg zeroes
static int km_assign_bf16_impl(const float* X, const void* Xb, const float* xnorm, int64_t N, int D, int ldx, const float* C, const void* Cb,
                               const float* cnorm, int K, int ldc, int32_t* labels, const int32_t* labels_old, int32_t* n_changed,
                               int32_t* stats, void* workspace, void* stream, int32_t* bc, int32_t* z0 = nullptr, int32_t* z1 = nullptr) {
  SLIC_REQUIRE(X && Xb && xnorm && C && Cb && cnorm && labels && workspace, "slic_kmeans_assign_bf16: null pointer");
  SLIC_REQUIRE(km_bf16_domain(N, K, D), "slic_kmeans_assign_bf16: the bf16 E-step takes D %% 8 == 0, D <= 512, N < 2^31 (N=%lld K=%d D=%d); "
               "use the fp32 entry point outside it", (long long)N, K, D);
  SLIC_REQUIRE(ldx % 4 == 0 && ldc % 4 == 0 && ldx >= D && ldc >= D, "slic_kmeans_assign_bf16: need 16-byte aligned rows (D=%d ldx=%d ldc=%d)", D, ldx, ldc);
  SLIC_REQUIRE(((uintptr_t)X % 16) == 0 && ((uintptr_t)C % 16) == 0 && ((uintptr_t)Xb % 16) == 0 && ((uintptr_t)Cb % 16) == 0,
               "slic_kmeans_assign_bf16: unaligned");
  SLIC_REQUIRE(!labels_old || n_changed, "slic_kmeans_assign_bf16: labels_old needs n_changed");
  const int cus = slic_device_cus();
  if (!cus) {
    slic_set_error("slic_kmeans_assign_bf16: cannot query the device's compute units");
    return SLIC_EHIP;
  }
  hipStream_t st = S_(stream);
  const int Dp = km_bf16_dp(D), Df = Dp / 2;
  const int ncb = (int)slic_cdiv(K, 128);
  const int64_t tiles = slic_cdiv(N, 128);
  // km_assign_creg's grid: blocks x slices covers the device once; a slice also has to fit one buffer resource (2^31 bytes)
  int64_t slices = ncb <= cus ? cus / ncb : 1;
  const int64_t need = slic_cdiv(N * (int64_t)Df * 4, 1ll << 30);
  if (slices < need) slices = need;
  if (slices > tiles) slices = tiles;
  SLIC_REQUIRE((slic_cdiv(tiles, slices) * 128 + 128) * (int64_t)Df * 4 < (1ll << 31), "slic_kmeans_assign_bf16: N too large");
  SlicCarver w(workspace);
  float* pub = w.take<float>((size_t)ncb * N);
  int32_t* pcnt = w.take<int32_t>((size_t)ncb * N);
  float* plo = w.take<float>((size_t)ncb * N);
  unsigned long long* cand = w.take<unsigned long long>((size_t)ncb * KMB_CAP * N);
  float* rowub = w.take<float>((size_t)N);
  uint32_t* list = w.take<uint32_t>((size_t)N);
  int32_t* nlist = w.take<int32_t>(64);
  {
    const size_t lds = (size_t)4 * SLIC_RT_TILE * sizeof(float) + 3 * 4 * 128 * sizeof(float);      // the ring + xch, wcnt, xlo
    const auto kern = Dp > 256 ? km_assign_bf16<8> : km_assign_bf16<4>;
    SLIC_LDS_LIMIT(kern, lds);
    kern<<<dim3((unsigned)slices, (unsigned)ncb), dim3(256), lds, st>>>((const float*)Xb, xnorm, N, Df, D, (const float*)Cb, K, cnorm, pub, pcnt,
                                                                       plo, cand, z0, z1, nlist);
    SLIC_LAUNCH_CHECK();
  }
  const bool hist = bc && (size_t)K * 4 <= 48 * 1024;
  if (hist)
    km_bf16_combine<true><<<dim3((unsigned)slic_cdiv(N, KM_SB)), dim3(KM_SB), (size_t)K * 4, st>>>(pub, pcnt, plo, cand, ncb, N, K, labels, labels_old,
                                                                                                n_changed, bc, rowub, list, nlist, stats);
  else
    km_bf16_combine<false><<<dim3((unsigned)slic_cdiv(N, 256)), dim3(256), 0, st>>>(pub, pcnt, plo, cand, ncb, N, K, labels, labels_old, n_changed,
                                                                                   nullptr, rowub, list, nlist, stats);
  SLIC_LAUNCH_CHECK();
  {
    int64_t nb = slic_cdiv(N, 4);
    if (nb > 8 * (int64_t)cus) nb = 8 * (int64_t)cus;                // the waves stride over the list
    km_bf16_rescore<<<dim3((unsigned)nb), dim3(256), 0, st>>>(X, N, D, ldx, C, K, ldc, cnorm, ncb, pcnt, cand, rowub, list, nlist, labels,
                                                             labels_old, n_changed, hist ? bc : nullptr);
    SLIC_LAUNCH_CHECK();
  }
  if (bc && !hist) {
    km_block_hist<<<dim3((unsigned)slic_cdiv(N, KM_SB)), dim3(KM_SB), (size_t)K * 4, st>>>(labels, N, K, bc);
    SLIC_LAUNCH_CHECK();
  }
  return SLIC_OK;
}

extern "C" int slic_kmeans_assign_bf16(const float* X, const void* Xb, const float* xnorm, int64_t N, int D, int ldx, const float* C,
                                       const void* Cb, const float* cnorm, int K, int ldc, int32_t* labels, const int32_t* labels_old,
                                       int32_t* n_changed, int32_t* stats, void* workspace, void* stream) {
  return km_assign_bf16_impl(X, Xb, xnorm, N, D, ldx, C, Cb, cnorm, K, ldc, labels, labels_old, n_changed, stats, workspace, stream, nullptr);
}

extern "C" size_t slic_kmeans_lloyd_step_bf16_workspace_bytes(int64_t N, int K) {
  return slic_align_up(slic_kmeans_assign_bf16_workspace_bytes(N, K), 256) + slic_kmeans_accumulate_workspace_bytes(N, K);
}

// the centres' image of this iteration: K x Dp values, one small launch
static int km_bf16_centre_image(const float* C, int K, int D, void* Cb, hipStream_t st) {
  const int Dp = km_bf16_dp(D);
  tkb_convert<<<dim3((unsigned)slic_cdiv((int64_t)K * (Dp / 8), 256)), dim3(256), 0, st>>>(C, K, D, D, Dp, (uint4*)Cb);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_kmeans_lloyd_step_bf16(const float* X, const float* Xp, const void* Xb, const float* xnorm, int64_t N, int D, int ldx,
                                           const float* C_old, void* Cb, const float* cnorm_old, int K, int32_t* labels,
                                           const int32_t* labels_old, int32_t* n_changed, float* sums, float* counts, float* C_new,
                                           float* Cp_new, float* cnorm_new, float* shift, int spherical, double* status, int32_t* stats,
                                           void* workspace, void* stream) {
  SLIC_REQUIRE(X && Xp && Xb && xnorm && C_old && Cb && cnorm_old && labels && n_changed && sums && counts && C_new && Cp_new && cnorm_new &&
               shift && status && workspace, "slic_kmeans_lloyd_step_bf16: null pointer");
  SLIC_REQUIRE(C_new != sums && C_new != C_old, "slic_kmeans_lloyd_step_bf16: C_new must not alias");
  SLIC_REQUIRE(km_bf16_domain(N, K, D), "slic_kmeans_lloyd_step_bf16: the bf16 E-step takes D %% 8 == 0, D <= 512 (N=%lld K=%d D=%d)", (long long)N, K, D);
  char* ws = (char*)workspace;
  void* ws2 = ws + slic_align_up(slic_kmeans_assign_bf16_workspace_bytes(N, K), 256);
  int rc = km_bf16_centre_image(C_old, K, D, Cb, S_(stream));
  if (rc) return rc;
  rc = km_assign_bf16_impl(X, Xb, xnorm, N, D, ldx, C_old, Cb, cnorm_old, K, D, labels, labels_old, n_changed, stats, ws, stream,
                           km_accumulate_hist_slab(ws2), n_changed, km_accumulate_done_counter(ws2, N, K));
  if (rc) return rc;
  KmFinish fin = {C_old, C_new, shift, cnorm_new, Cp_new, spherical, status, false};
  rc = km_accumulate_impl<float>(Xp, N, D, ldx, labels, K, sums, counts, n_changed, nullptr, ws2, stream, true, &fin, 1);
  if (rc || fin.done) return rc;
  return slic_kmeans_finalize(C_old, sums, counts, K, D, C_new, shift, cnorm_new, Cp_new, spherical, n_changed, status, stream);
}

extern "C" size_t slic_kmeans_lloyd_local_bf16_workspace_bytes(int64_t N, int K) {
  return slic_kmeans_lloyd_step_bf16_workspace_bytes(N, K) + 256;
}

extern "C" int slic_kmeans_lloyd_local_bf16(const float* X, const float* Xp, const void* Xb, const float* xnorm, int64_t N, int D, int ldx,
                                            const float* C_old, void* Cb, const float* cnorm_old, int K, int32_t* labels,
                                            const int32_t* labels_old, void* payload, int payload_f64, int32_t* stats, void* workspace,
                                            void* stream) {
  SLIC_REQUIRE(X && Xp && Xb && xnorm && C_old && Cb && cnorm_old && labels && payload && workspace, "slic_kmeans_lloyd_local_bf16: null pointer");
  SLIC_REQUIRE(km_bf16_domain(N, K, D), "slic_kmeans_lloyd_local_bf16: the bf16 E-step takes D %% 8 == 0, D <= 512 (N=%lld K=%d D=%d)", (long long)N, K, D);
  char* ws = (char*)workspace;
  void* ws2 = ws + slic_align_up(slic_kmeans_assign_bf16_workspace_bytes(N, K), 256);
  int32_t* n_changed = (int32_t*)(ws + slic_kmeans_lloyd_step_bf16_workspace_bytes(N, K));
  int rc = km_bf16_centre_image(C_old, K, D, Cb, S_(stream));
  if (rc) return rc;
  const bool small = km_small_shard(N, D, ldx);
  rc = km_assign_bf16_impl(X, Xb, xnorm, N, D, ldx, C_old, Cb, cnorm_old, K, D, labels, labels_old, n_changed, stats, ws, stream,
                           small ? nullptr : km_accumulate_hist_slab(ws2), n_changed);
  if (rc) return rc;
  const int64_t KD = (int64_t)K * D;
  if (payload_f64) {
    double* p = (double*)payload;
    return km_accumulate_impl<double>(Xp, N, D, ldx, labels, K, p, p + KD, n_changed, p + KD + K, ws2, stream, !small, nullptr, 1);
  }
  float* p = (float*)payload;
  return km_accumulate_impl<float>(Xp, N, D, ldx, labels, K, p, p + KD, n_changed, p + KD + K, ws2, stream, !small, nullptr, 1);
}
