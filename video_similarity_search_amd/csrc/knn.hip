// What one does with a top-k list besides hit@k: the weighted k-NN vote (sklearn's KNeighborsClassifier, the k-NN monitor of
// InstDisc / MoCo / DINO) and the ranked retrieval metrics (precision@K, recall@K, AP@K, reciprocal rank), on the [Nq, k] index and
// distance tables as slic_cosine_topk / slic_euclidean_topk / slic_topk_merge_lists write them.  The contract, the weight rules and
// the summation orders are in include/slic_hip.h (slic_knn_vote, slic_retrieval_ranked).
//
//   knn_vote_kernel          : one wave per query, four per workgroup.  The wave's C class scores live in its own slab of LDS.  A chunk
//                              of 64 table entries goes to the lanes (the label gather runs 64 wide); the votes are then added ONE AT A
//                              TIME in rank order by lane 0 (entry j is broadcast with readlane): a class's score is the float32 sum of
//                              its neighbours' weights in rank order, which is what a sequential restatement computes.  The total over
//                              the classes and the n_top arg-max rounds are xor butterflies over per-lane partials in class order.
//   retrieval_ranked_kernel  : one wave per query.  Hit flags per chunk of 64, their inclusive prefix sums by the __shfl_up ladder with a
//                              carry between chunks, the AP terms c_j / (j + 1) scanned the same way in double; a cut-off K reads lane
//                              (K - 1) & 63 of chunk (K - 1) / 64.
//   retrieval_mean_kernel    : one workgroup per column of the per-query table: thread t adds queries t, t + 256, ... in ascending order,
//                              slic_wg_fold adds the 256 partials.  Double, a fixed order, no atomics.
// fp contraction is off for the whole file: the test restates every operation as a separately rounded one.
#include "wg_scan.h"
#include <math.h>

#pragma clang fp contract(off)

#define KNN_WAVES 4                 // waves (= queries) per workgroup
#define KNN_MEAN_T 256              // threads of a column sum

struct KnnCuts { int n; int k[SLIC_KNN_MAX_CUTS]; };

// (score, class) of two candidates: the higher score wins, the lower class among equals; class -1 = no candidate
__device__ __forceinline__ bool knn_better(float sa, int ca, float sb, int cb) {
  if (cb < 0) return ca >= 0;
  if (ca < 0) return false;
  return sa > sb || (sa == sb && ca < cb);
}

// the table entry (q, j) as a vote: its class (-1: it does not vote) and its distance
__device__ __forceinline__ int knn_entry(const int32_t* __restrict__ idx, const float* __restrict__ dist,
                                         const int64_t* __restrict__ g_labels, int Ng, int C, int64_t row, int j, int k, bool live,
                                         float* d) {
  int c = -1;
  *d = 0.f;
  if (live && j < k) {
    const int32_t g = idx[row + j];
    if (g >= 0 && g < Ng) {
      const int64_t l = g_labels[g];
      if (l >= 0 && l < (int64_t)C) {
        c = (int)l;
        if (dist) *d = dist[row + j];
      }
    }
  }
  return c;
}

__global__ __launch_bounds__(KNN_WAVES * 64) void knn_vote_kernel(
    const int32_t* __restrict__ idx, const float* __restrict__ dist, int Nq, int k, const int64_t* __restrict__ g_labels, int Ng, int C,
    int mode, float inv_t, int n_top, float* __restrict__ proba, int32_t* __restrict__ pred, float* __restrict__ score) {
  extern __shared__ float knn_lds[];                         // KNN_WAVES slabs of C floats; nothing else lives in LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * KNN_WAVES + wave;
  const bool live = q < Nq;                                  // a dead wave walks the same path with nothing voting: the barriers are uniform
  const int64_t row = (int64_t)(live ? q : 0) * k;
  float* sc = knn_lds + (size_t)wave * C;

  for (int c = lane; c < C; c += 64) sc[c] = 0.f;

  // what the weights need from the whole row: is there a voting neighbour at distance 0 (mode 1), the first voting distance (mode 2)
  bool any_zero = false;
  float d0 = 0.f;
  if (mode != SLIC_KNN_UNIFORM) {
    bool have_d0 = false;
    for (int j0 = 0; j0 < k; j0 += 64) {
      float d;
      const int c = knn_entry(idx, dist, g_labels, Ng, C, row, j0 + lane, k, live, &d);
      const unsigned long long votes = __ballot(c >= 0);
      any_zero = any_zero || __ballot(c >= 0 && d == 0.f) != 0ull;
      if (!have_d0 && votes != 0ull) {
        d0 = __shfl(d, __ffsll((long long)votes) - 1);
        have_d0 = true;
      }
    }
  }
  __syncthreads();

  bool voted = false;
  for (int j0 = 0; j0 < k; j0 += 64) {
    float d;
    const int c = knn_entry(idx, dist, g_labels, Ng, C, row, j0 + lane, k, live, &d);
    float w = 1.f;
    if (mode == SLIC_KNN_DISTANCE) w = any_zero ? (d == 0.f ? 1.f : 0.f) : 1.f / d;
    else if (mode == SLIC_KNN_SOFTMAX) w = expf((d0 - d) * inv_t);
    const unsigned long long votes = __ballot(c >= 0);
    voted = voted || votes != 0ull;
    const int n = min(64, k - j0);
    for (int j = 0; j < n; ++j) {                            // rank order: one vote at a time, all by lane 0
      const int cj = __builtin_amdgcn_readlane(c, j);
      const float wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), j));
      if (cj >= 0 && lane == 0) sc[cj] += wj;
    }
  }
  __syncthreads();

  // the total: lane l adds classes l, l + 64, ... ascending, then the xor butterfly 32, 16, .. 1
  float tot = 0.f;
  for (int c = lane; c < C; c += 64) tot += sc[c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);

  if (proba && live) {
    float* p = proba + (int64_t)q * C;
    for (int c = lane; c < C; c += 64) p[c] = voted ? sc[c] / tot : 0.f;
  }
  if (n_top == 0) return;                                    // uniform: no barrier follows for anybody
  __syncthreads();                                           // every lane has read the scores it divides before a winner is struck out

  for (int r = 0; r < n_top; ++r) {
    float bs = 0.f;
    int bc = -1;
    if (voted) {
      for (int c = lane; c < C; c += 64) {
        const float s = sc[c];
        if (s >= 0.f && knn_better(s, c, bs, bc)) { bs = s; bc = c; }     // a struck-out class holds -1
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o);
      const int oc = __shfl_xor(bc, o);
      if (knn_better(os, oc, bs, bc)) { bs = os; bc = oc; }
    }
    if (live && lane == 0) {
      if (pred) pred[(int64_t)q * n_top + r] = bc;
      if (score) score[(int64_t)q * n_top + r] = bc >= 0 ? bs : 0.f;
    }
    if (bc >= 0 && lane == (bc & 63)) sc[bc] = -1.f;
    __syncthreads();
  }
}

extern "C" int slic_knn_vote(const int32_t* idx, const float* dist, int Nq, int k, const int64_t* g_labels, int Ng, int C, int mode,
                             float temperature, int n_top, float* proba, int32_t* pred, float* score, void* stream) {
  SLIC_REQUIRE(idx && g_labels, "slic_knn_vote: null pointer");
  SLIC_REQUIRE(Nq >= 1 && Ng >= 1, "slic_knn_vote: Nq = %d, Ng = %d (both must be >= 1)", Nq, Ng);
  SLIC_REQUIRE(k >= 1 && k <= SLIC_KNN_MAX_K, "slic_knn_vote: k = %d (1 .. %d)", k, SLIC_KNN_MAX_K);
  SLIC_REQUIRE(C >= 1 && C <= SLIC_KNN_MAX_CLASSES, "slic_knn_vote: C = %d (1 .. %d)", C, SLIC_KNN_MAX_CLASSES);
  SLIC_REQUIRE(mode == SLIC_KNN_UNIFORM || mode == SLIC_KNN_DISTANCE || mode == SLIC_KNN_SOFTMAX, "slic_knn_vote: mode = %d (0, 1, 2)", mode);
  SLIC_REQUIRE(mode == SLIC_KNN_UNIFORM || dist, "slic_knn_vote: mode %d needs the distance table", mode);
  SLIC_REQUIRE(mode != SLIC_KNN_SOFTMAX || temperature > 0.f, "slic_knn_vote: temperature = %g (must be > 0)", (double)temperature);
  SLIC_REQUIRE(n_top >= 0 && n_top <= SLIC_KNN_MAX_TOP, "slic_knn_vote: n_top = %d (0 .. %d)", n_top, SLIC_KNN_MAX_TOP);
  SLIC_REQUIRE(n_top > 0 ? (pred || score) : (!pred && !score), "slic_knn_vote: n_top = %d does not go with the pred / score pointers given", n_top);
  SLIC_REQUIRE(proba || n_top > 0, "slic_knn_vote: no output asked for");
  const size_t lds = (size_t)KNN_WAVES * (size_t)C * sizeof(float);       // at most 64 KB: the default limit
  knn_vote_kernel<<<dim3((unsigned)slic_cdiv(Nq, KNN_WAVES)), dim3(KNN_WAVES * 64), lds, S_(stream)>>>(
      idx, dist, Nq, k, g_labels, Ng, C, mode, mode == SLIC_KNN_SOFTMAX ? 1.f / temperature : 0.f, n_top, proba, pred, score);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

// per_query[q, i, 0 .. 2] = (P@K_i, R@K_i, AP@K_i), rr[q] = the reciprocal rank
__global__ __launch_bounds__(KNN_WAVES * 64) void retrieval_ranked_kernel(
    const int32_t* __restrict__ idx, int Nq, int k, const int64_t* __restrict__ q_labels, const int64_t* __restrict__ g_labels, int Ng,
    const int32_t* __restrict__ n_rel, KnnCuts ks, double* __restrict__ per_query, double* __restrict__ rr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * KNN_WAVES + wave;
  if (q >= Nq) return;                                       // no barrier in this kernel: a whole wave may leave
  const int64_t ql = q_labels[q];
  const int nr = n_rel[q];
  const int32_t* row = idx + (int64_t)q * k;
  int carry = 0, first = -1, next = 0;                       // next: the first cut-off not yet written
  double ap_carry = 0.0;
  for (int j0 = 0; j0 < k && next < ks.n; j0 += 64) {
    const int j = j0 + lane;
    bool h = false;
    if (j < k) {
      const int32_t g = row[j];
      h = g >= 0 && g < Ng && g_labels[g] == ql;             // padding (-1) and rows past the gallery never hit
    }
    const unsigned long long hits = __ballot(h);
    if (first < 0 && hits != 0ull) first = j0 + __ffsll((long long)hits) - 1;
    int c = h ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(c, o);
      if (lane >= o) c += u;
    }
    c += carry;                                              // c_j
    double a = h ? (double)c / (double)(j + 1) : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_up(a, o);
      if (lane >= o) a += u;
    }
    a = ap_carry + a;                                        // sum_{j' <= j, h_j'} c_j' / (j' + 1)
    while (next < ks.n && ks.k[next] <= j0 + 64) {           // cut-offs inside this chunk (ks.k <= k: the lane they read is a table entry)
      const int K = ks.k[next], src = (K - 1) & 63;
      const int cK = __shfl(c, src);
      const double aK = __shfl(a, src);
      if (lane == 0) {
        double* o = per_query + ((int64_t)q * ks.n + next) * 3;
        o[0] = (double)cK / (double)K;
        o[1] = nr > 0 ? (double)cK / (double)nr : 0.0;
        o[2] = nr > 0 ? aK / (double)min(nr, K) : 0.0;
      }
      ++next;
    }
    carry = __shfl(c, 63);
    ap_carry = __shfl(a, 63);
  }
  // the reciprocal rank looks at the whole row, also past the last cut-off
  for (int j0 = (ks.k[ks.n - 1] + 63) / 64 * 64; first < 0 && j0 < k; j0 += 64) {
    const int j = j0 + lane;
    bool h = false;
    if (j < k) {
      const int32_t g = row[j];
      h = g >= 0 && g < Ng && g_labels[g] == ql;
    }
    const unsigned long long hits = __ballot(h);
    if (hits != 0ull) first = j0 + __ffsll((long long)hits) - 1;
  }
  if (lane == 0) rr[q] = first >= 0 ? 1.0 / (double)(first + 1) : 0.0;
}

// block b < 3 * n_ks: the mean of column b of per_query; block 3 * n_ks: the mean of rr; every block counts the queries with relevant rows,
// block 0 writes the count.  Recall and AP (columns 1, 2 of a cut-off) leave the queries with n_rel == 0 out of sum and divisor.
__global__ __launch_bounds__(KNN_MEAN_T) void retrieval_mean_kernel(const double* __restrict__ per_query, const double* __restrict__ rr,
                                                                   const int32_t* __restrict__ n_rel, int Nq, int n_ks,
                                                                   double* __restrict__ record) {
  __shared__ double s[KNN_MEAN_T];
  const int b = blockIdx.x, cols = 3 * n_ks;
  const bool is_rr = b == cols;
  const bool relevant_only = !is_rr && (b % 3) != 0;
  double acc = 0.0, cnt = 0.0;
  for (int q = threadIdx.x; q < Nq; q += KNN_MEAN_T) {
    const bool rel = n_rel[q] > 0;
    if (rel) cnt += 1.0;
    if (rel || !relevant_only) acc += is_rr ? rr[q] : per_query[(int64_t)q * cols + b];
  }
  const double sum = slic_wg_fold<KNN_MEAN_T>(acc, s);
  const double n = slic_wg_fold<KNN_MEAN_T>(cnt, s);          // whole numbers below 2^53: exact in any order
  if (threadIdx.x == 0) {
    const double div = relevant_only ? n : (double)Nq;
    record[b] = div > 0.0 ? sum / div : 0.0;
    if (b == 0) record[cols + 1] = n;
  }
}

extern "C" int slic_retrieval_ranked(const int32_t* idx, int Nq, int k, const int64_t* q_labels, const int64_t* g_labels, int Ng,
                                     const int32_t* n_rel, const int32_t* cutoffs, int n_ks, double* per_query, double* rr,
                                     double* record, void* stream) {
  SLIC_REQUIRE(idx && q_labels && g_labels && n_rel && cutoffs && per_query && rr, "slic_retrieval_ranked: null pointer");
  SLIC_REQUIRE(Nq >= 1 && Ng >= 1, "slic_retrieval_ranked: Nq = %d, Ng = %d (both must be >= 1)", Nq, Ng);
  SLIC_REQUIRE(k >= 1 && k <= SLIC_KNN_MAX_K, "slic_retrieval_ranked: k = %d (1 .. %d)", k, SLIC_KNN_MAX_K);
  SLIC_REQUIRE(n_ks >= 1 && n_ks <= SLIC_KNN_MAX_CUTS, "slic_retrieval_ranked: n_ks = %d (1 .. %d)", n_ks, SLIC_KNN_MAX_CUTS);
  KnnCuts ks;
  ks.n = n_ks;
  for (int i = 0; i < SLIC_KNN_MAX_CUTS; ++i) ks.k[i] = i < n_ks ? cutoffs[i] : 0;
  for (int i = 0; i < n_ks; ++i)
    SLIC_REQUIRE(ks.k[i] >= 1 && ks.k[i] <= k && (i == 0 || ks.k[i] >= ks.k[i - 1]),
                 "slic_retrieval_ranked: cutoffs must be ascending and in 1 .. k = %d (cutoffs[%d] = %d)", k, i, ks.k[i]);
  hipStream_t s = S_(stream);
  retrieval_ranked_kernel<<<dim3((unsigned)slic_cdiv(Nq, KNN_WAVES)), dim3(KNN_WAVES * 64), 0, s>>>(idx, Nq, k, q_labels, g_labels, Ng,
                                                                                                  n_rel, ks, per_query, rr);
  SLIC_LAUNCH_CHECK();
  if (record) {
    retrieval_mean_kernel<<<dim3((unsigned)(3 * n_ks + 1)), dim3(KNN_MEAN_T), 0, s>>>(per_query, rr, n_rel, Nq, n_ks, record);
    SLIC_LAUNCH_CHECK();
  }
  return SLIC_OK;
}
