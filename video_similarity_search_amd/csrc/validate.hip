// The per-batch arithmetic of the validation pass (validation.py:59-71 and evaluate.py:296-305 of the reference) on the device.
//
//   triplet_val_batch_kernel : after the three encoder passes — dist_a = d(x, y), dist_b = d(x, z) per row (pairdist.h: the bits of
//                              slic_pair_distance), MarginRankingLoss(margin)(dist_a, dist_b, -1) with mean reduction, and the
//                              accuracy #{dist_b - dist_a > 0} / B — as ONE launch that writes one row of the epoch record.
//   topk_label_hits_kernel   : get_topk_acc's double loop on a [Nq, k] index table that is already on the device: per query the first
//                              column whose gallery label equals the query's, per top-k the number of queries that hit inside it.
#include "common.h"
#include "pairdist.h"

#define VAL_WAVES 16                 // waves of the one workgroup: a validation batch is at most a few hundred rows
#define VAL_CHUNK 256                // floats of a row a wave stages per step (64 lanes x 16 bytes)

// ONE workgroup; wave w takes rows w, w + 16, ...  A row's elements go to the lanes as pairdist.h says (lane l: l, l + 64, ...).  With
// VEC the wave fetches 256 consecutive floats of each of the three rows with one 16-byte load per lane, parks them in its own LDS
// slab and every lane picks its four elements from there (stride-64 reads: conflict free), so the sums see the same elements in the
// same order as on the scalar path.  x is read once for both distances.
// The hinge terms are summed in double: per wave in row order, then the 16 wave sums in wave order by thread 0 — a fixed order, no
// atomics, and the float result is the correctly rounded mean whatever B is.
template <bool VEC>
__global__ __launch_bounds__(VAL_WAVES * 64) void triplet_val_batch_kernel(
    const float* __restrict__ X, const float* __restrict__ Y, const float* __restrict__ Z, int B, int D, int euclid, float margin,
    float* __restrict__ dist_a, float* __restrict__ dist_b, float* __restrict__ rec) {
  __shared__ __attribute__((aligned(16))) float stage[VEC ? VAL_WAVES : 1][3][VAL_CHUNK];
  __shared__ double wsum[VAL_WAVES];
  __shared__ int wcnt[VAL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double hsum = 0.0;
  int cnt = 0;
  for (int r0 = 0; r0 < B; r0 += VAL_WAVES) {          // every wave makes every trip: the barriers below are uniform
    const int row = r0 + wave;
    const bool live = row < B;
    const float* x = X + (int64_t)(live ? row : 0) * D;
    const float* y = Y + (int64_t)(live ? row : 0) * D;
    const float* z = Z + (int64_t)(live ? row : 0) * D;
    float a1 = 0.f, b = 0.f, c1 = 0.f, a2 = 0.f, b2 = 0.f, c2 = 0.f;   // b2 mirrors b: slic_pd_step keeps the pair's own x.x
    if (VEC) {
      for (int k0 = 0; k0 < D; k0 += VAL_CHUNK) {
        const int k4 = k0 + 4 * lane;
        if (live && k4 < D) {                          // D % 4 == 0: a lane's four floats are inside the row or all outside
          *(f32x4*)&stage[wave][0][4 * lane] = *(const f32x4*)(x + k4);
          *(f32x4*)&stage[wave][1][4 * lane] = *(const f32x4*)(y + k4);
          *(f32x4*)&stage[wave][2][4 * lane] = *(const f32x4*)(z + k4);
        }
        __syncthreads();
        if (live) {
#pragma unroll
          for (int i = 0; i < VAL_CHUNK / 64; ++i) {
            const int k = k0 + lane + 64 * i;
            if (k < D) {
              const float xv = stage[wave][0][lane + 64 * i];
              slic_pd_step(xv, stage[wave][1][lane + 64 * i], euclid, a1, b, c1);
              slic_pd_step(xv, stage[wave][2][lane + 64 * i], euclid, a2, b2, c2);
            }
          }
        }
        __syncthreads();                               // the slab is free for the next chunk
      }
    } else if (live) {
      for (int k = lane; k < D; k += 64) {
        const float xv = x[k];
        slic_pd_step(xv, y[k], euclid, a1, b, c1);
        slic_pd_step(xv, z[k], euclid, a2, b2, c2);
      }
    }
    slic_pd_wave_sum(a1, b, c1);
    slic_pd_wave_sum(a2, b2, c2);
    if (live && lane == 0) {
      const float da = slic_pd_finish(a1, b, c1, euclid), db = slic_pd_finish(a2, b2, c2, euclid);
      if (dist_a) dist_a[row] = da;
      if (dist_b) dist_b[row] = db;
      hsum += (double)fmaxf((da - db) + margin, 0.f);   // (-target * (input1 - input2) + margin).clamp_min(0), target = -1
      cnt += (db - da) > 0.f ? 1 : 0;                   // accuracy(): pred = dist_b - dist_a - 0, pred > 0
    }
  }
  if (lane == 0) { wsum[wave] = hsum; wcnt[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int n = 0;
    for (int w = 0; w < VAL_WAVES; ++w) { s += wsum[w]; n += wcnt[w]; }
    rec[0] = (float)(s / (double)B);
    rec[1] = (float)n / (float)B;                       // (pred > 0).sum() * 1.0 / B in float32, as torch computes it
    rec[2] = (float)B;
  }
}

extern "C" int slic_triplet_val_batch(const float* ex, const float* ey, const float* ez, int B, int D, int euclid, float margin,
                                      float* dist_a, float* dist_b, float* rec, void* stream) {
  SLIC_REQUIRE(B >= 1 && D >= 1, "slic_triplet_val_batch: B = %d, D = %d (both must be >= 1)", B, D);
  SLIC_REQUIRE(ex && ey && ez && rec, "slic_triplet_val_batch: null pointer");
  SLIC_REQUIRE(B < (1 << 24), "slic_triplet_val_batch: B = %d does not fit the float32 record exactly", B);
  const bool vec = D % 4 == 0 && (((uintptr_t)ex | (uintptr_t)ey | (uintptr_t)ez) & 15) == 0;   // then every row start is aligned
  hipStream_t s = (hipStream_t)stream;
  if (vec) triplet_val_batch_kernel<true><<<dim3(1), dim3(VAL_WAVES * 64), 0, s>>>(ex, ey, ez, B, D, euclid, margin, dist_a, dist_b, rec);
  else triplet_val_batch_kernel<false><<<dim3(1), dim3(VAL_WAVES * 64), 0, s>>>(ex, ey, ez, B, D, euclid, margin, dist_a, dist_b, rec);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

struct TopKs { int n; int k[8]; };

// one thread per query walks its row of the table up to the first hit; per top-k a workgroup counts its hitting queries in LDS
// (ballot + popcount per wave, then 4 wave counts in order) and adds them to hits[] with ONE vector atomic on int32 — integer
// addition: the result does not depend on the order.  hits[] is zeroed on the stream before the launch.
__global__ __launch_bounds__(256) void topk_label_hits_kernel(const int32_t* __restrict__ idx, int Nq, int k,
                                                              const int64_t* __restrict__ q_labels,
                                                              const int64_t* __restrict__ g_labels, int Ng, TopKs ks,
                                                              int32_t* __restrict__ first_hit, int32_t* __restrict__ hits) {
  __shared__ int wcount[4][8];
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int first = k;
  if (q < Nq) {
    const int64_t ql = q_labels[q];
    const int32_t* row = idx + (int64_t)q * k;
    for (int j = 0; j < k; ++j) {
      const int32_t g = row[j];
      if (g >= 0 && g < Ng && g_labels[g] == ql) { first = j; break; }      // padding (-1) and rows past the gallery never hit
    }
    if (first_hit) first_hit[q] = first;
  }
  for (int i = 0; i < ks.n; ++i) {
    const unsigned long long m = __ballot(q < Nq && first < ks.k[i]);
    if (lane == 0) wcount[wave][i] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x < ks.n) {
    const int i = threadIdx.x;
    const int c = wcount[0][i] + wcount[1][i] + wcount[2][i] + wcount[3][i];
    if (c) atomicAdd(&hits[i], c);
  }
}

extern "C" int slic_topk_label_hits(const int32_t* idx, int Nq, int k, const int64_t* q_labels, const int64_t* g_labels, int Ng,
                                    const int32_t* top_ks, int n_ks, int32_t* first_hit, int32_t* hits, void* stream) {
  SLIC_REQUIRE(idx && q_labels && g_labels && top_ks && hits, "slic_topk_label_hits: null pointer");
  SLIC_REQUIRE(Nq >= 1 && k >= 1 && Ng >= 1, "slic_topk_label_hits: Nq = %d, k = %d, Ng = %d (all must be >= 1)", Nq, k, Ng);
  SLIC_REQUIRE(n_ks >= 1 && n_ks <= 8, "slic_topk_label_hits: n_ks = %d (1 .. 8)", n_ks);
  TopKs ks;
  ks.n = n_ks;
  for (int i = 0; i < 8; ++i) ks.k[i] = i < n_ks ? top_ks[i] : 0;
  for (int i = 0; i < n_ks; ++i)
    SLIC_REQUIRE(ks.k[i] >= 1 && ks.k[i] <= k && (i == 0 || ks.k[i] >= ks.k[i - 1]),
                 "slic_topk_label_hits: top_ks must be ascending and in 1 .. k = %d (top_ks[%d] = %d)", k, i, ks.k[i]);
  hipStream_t s = (hipStream_t)stream;
  SLIC_HIP_CHECK(hipMemsetAsync(hits, 0, (size_t)n_ks * sizeof(int32_t), s));
  topk_label_hits_kernel<<<dim3((unsigned)slic_cdiv(Nq, 256)), dim3(256), 0, s>>>(idx, Nq, k, q_labels, g_labels, Ng, ks, first_hit,
                                                                                 hits);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
