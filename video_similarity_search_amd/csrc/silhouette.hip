// Silhouette coefficient of a labelled set of rows on the device, for the two metrics whose sum of distances to a cluster is a
// function of the cluster's row sum ("Silhouette from cluster sums"; contract in include/slic_hip.h):
//   cosine        sum_{j in C} (1 - x^_i . x^_j)   = |C| - x^_i . S_C                       S_C = sum of the unit rows
//   sqeuclidean   sum_{j in C} |x_i - x_j|^2       = |C| |x_i|^2 - 2 x_i . S_C + Q_C        Q_C = sum of the squared norms
// so every row's mean distance to every cluster is one entry of rows [N, D] x means [K, D]^T: the k-means E-step's contraction on
// the shared MFMA row-tile ring (mfma_ring.h), with (own-cluster distance, min over the other clusters, its index) carried per row
// in place of (min, argmin).  No N x N and no N x K array exists.
//
// Passes (one stream, no host synchronisation: the number of clusters is read from `meta` on the device; the grids are sized by
// the caller's bound Kmax):
//   ids      dense ids 0 .. U - 1 by ascending label value, class sizes, and the rows in (id, row) order (label_ids.h: the
//            NMI / AMI call's sort, carrying the row number)
//   check    the ignored label's id, K, the rows scored, status
//   prep     per row: |x|^2 in float64 (k ascending); the operand row (x / |x| for cosine, a zero row stays zero; x for
//            sqeuclidean) rounded to fp32, zero-padded to D % 8 == 0 and stored in the ring's k order (km_permute_k8's); the self
//            term 1 - x^.x^ as the MFMA computes it (an fp32 fmaf chain, k ascending)
//   stats    per cluster: the float64 sum of its operand rows in ascending row order, divided by |C| and rounded ONCE to fp32 (the
//            mean the contraction reads); Q_C / |C| the same way.  (kmeans.hip's km_place / km_accumulate<double> do not give this: they
//            add in fp32 and only store widened, and their grids and LDS need K on the host.)
//   score    sil_score: 128 rows x 64 clusters per tile, both operands by DMA, 2 stages (km_assign_dma's tile and ring); a workgroup
//            owns a row tile and walks a contiguous share of the cluster tiles (grid.y shares: the K-group split), the ring running
//            on across tiles
//   finish   combines the shares in ascending order (strict '<': the first dense id wins), a = own / (|C| - 1), b, s; writes the rows
//   means    per-cluster and overall means of s in float64, in a fixed order (strided partial sums folded by halving: slic_wg_fold)
// fp contraction is off for the whole file (Makefile: FLAGS_silhouette): every fused multiply-add is spelled fmaf, which is what the
// test mirror restates.
#include "label_ids.h"
#include "mfma_ring.h"
#include "wg_scan.h"
#include <math.h>

#define SIL_T 256
#define SIL_G 1024            // workgroups of the fixed-order sum of s
#define SIL_BP 128            // rows per workgroup of the score kernel
#define SIL_NCT 2             // 32-cluster MFMA tiles per cluster tile
#define SIL_BC (SIL_NCT * 32)
#define SIL_ST 2              // ring stages
#define SIL_MAX_SPLIT 8       // K-group shares

enum { SIL_U = 0, SIL_IG = 1, SIL_K = 2, SIL_NEFF = 3, SIL_STATUS = 4, SIL_NMETA = 16 };

__global__ void sil_check(const uint32_t* __restrict__ uniq, const int* __restrict__ cnt, int N, int has_ignore, int32_t ignore_label,
                          int kcap, int kmax, int* __restrict__ meta) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int U = min(meta[SIL_U], N);
  int ig = -1;
  if (has_ignore) {
    const uint32_t key = (uint32_t)ignore_label ^ 0x80000000u;
    int lo = 0, hi = U;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (uniq[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < U && uniq[lo] == key) ig = lo;
  }
  const int K = U - (ig >= 0 ? 1 : 0);
  const int neff = N - (ig >= 0 ? cnt[ig] : 0);
  meta[SIL_U] = U;
  meta[SIL_IG] = ig;
  meta[SIL_K] = K;
  meta[SIL_NEFF] = neff;
  meta[SIL_STATUS] = (K < 2 || K > neff - 1) ? SLIC_SILHOUETTE_UNDEFINED : (U > kcap || K > kmax) ? SLIC_SILHOUETTE_TOO_MANY : 0;
}

// position of natural column k in the ring's k order: inside every group of eight, [k0 k2 k4 k6 | k1 k3 k5 k7]
__device__ __forceinline__ int sil_perm(int k) { return (k & ~7) + ((k & 1) << 2) + ((k & 7) >> 1); }

__global__ __launch_bounds__(SIL_T) void sil_prep(const float* __restrict__ X, int N, int D, int64_t ldx, int Dp, int cosine,
                                                 float* __restrict__ xp, float* __restrict__ xnf, float* __restrict__ selft,
                                                 double* __restrict__ xn64) {
  const int i = blockIdx.x * SIL_T + threadIdx.x;
  if (i >= N) return;
  const float* x = X + (int64_t)i * ldx;
  float* o = xp + (int64_t)i * Dp;
  double n2 = 0.0;
  for (int k = 0; k < D; ++k) n2 += (double)x[k] * (double)x[k];
  const double nrm = sqrt(n2);
  float dot = 0.f;
  for (int k = 0; k < D; ++k) {
    const float v = cosine ? (nrm > 0.0 ? (float)((double)x[k] / nrm) : 0.f) : x[k];
    o[sil_perm(k)] = v;
    dot = fmaf(v, v, dot);
  }
  for (int k = D; k < Dp; ++k) o[sil_perm(k)] = 0.f;
  xn64[i] = n2;
  xnf[i] = cosine ? 0.f : (float)n2;
  selft[i] = cosine ? 1.0f - dot : 0.f;
}

__global__ __launch_bounds__(SIL_T) void sil_fill(float* __restrict__ p, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * SIL_T + threadIdx.x;
  if (i < n) p[i] = v;
}

// cluster u's mean operand row and its column term: thread = one column (column Dp: the squared norms); rows in ascending order
__global__ __launch_bounds__(64) void sil_stats(const float* __restrict__ xp, const double* __restrict__ xn64, int Dp, int cosine,
                                                const int* __restrict__ ord, const int* __restrict__ start, const int* __restrict__ cnt,
                                                const int* __restrict__ meta, float* __restrict__ mp, float* __restrict__ colq) {
  const int u = blockIdx.x;
  if (meta[SIL_STATUS] || u >= meta[SIL_U]) return;
  const int col = blockIdx.y * 64 + threadIdx.x;
  if (col > Dp) return;
  const int n = cnt[u];
  const int* o = ord + start[u];
  const bool ignored = u == meta[SIL_IG];                     // its column never wins and is nobody's own: +inf over a zero mean
  if (ignored || (col == Dp && cosine)) {
    if (col == Dp) colq[u] = ignored ? INFINITY : 1.0f;
    else mp[(int64_t)u * Dp + col] = 0.f;                     // (a finite dot product keeps fmaf(-alpha, dot, +inf) at +inf)
    return;
  }
  // eight loads in flight; the float64 sum stays in ascending row order
  auto at = [&](int m) -> double { return col == Dp ? xn64[o[m]] : (double)xp[(int64_t)o[m] * Dp + col]; };
  double acc = 0.0;
  int m = 0;
  for (; m + 8 <= n; m += 8) {
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = at(m + t);
#pragma unroll
    for (int t = 0; t < 8; ++t) acc += v[t];
  }
  for (; m < n; ++m) acc += at(m);
  const float mean = (float)(acc / (double)n);
  if (col == Dp) colq[u] = mean;
  else mp[(int64_t)u * Dp + col] = mean;
}

// Per row i and share y of the cluster tiles: the distance to the row's own cluster (-1 when the share does not hold it), the
// smallest distance to another cluster and that cluster's dense id.  distance(i, c) = max(fmaf(-alpha, x_i . m_c, xn_i + q_c), 0):
// cosine alpha = 1, xn = 0, q = 1; sqeuclidean alpha = 2, xn = |x_i|^2, q = Q_c / |C|; q = +inf for a column that is no cluster.
// MFMA roles, LDS image, DMA addressing and the ring are km_assign_dma<128, 2, 1, 2>'s: A = cluster tile, B = row tile, so a lane
// holds ONE row (32 wave + (lane & 31)) and accumulator element g of tile ct is cluster 32 ct + (g & 3) + 8 (g >> 2) + 4 (lane >> 5).
// Rows past N, clusters past U and k-tiles past D lie outside a buffer resource's range or are sent there: zeros, exact no-ops.
__global__ __launch_bounds__(256) void sil_score(const float* __restrict__ xp, int N, int Dp, const float* __restrict__ mp,
                                                 const float* __restrict__ colq, const float* __restrict__ xnf,
                                                 const int* __restrict__ ids, const int* __restrict__ meta, float alpha,
                                                 float* __restrict__ pown, float* __restrict__ pbest, int* __restrict__ pidx) {
  extern __shared__ __attribute__((aligned(16))) float sil_lds[];
  if (meta[SIL_STATUS]) return;
  constexpr int STAGE_FLOATS = (SIL_BP + SIL_BC) * SLIC_RT_BK;
  constexpr int PER_STAGE = SIL_BP / 32 + SIL_NCT;
  const int U = meta[SIL_U], ig = meta[SIL_IG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int pblock = blockIdx.x * SIL_BP;
  const int tiles = (U + SIL_BC - 1) / SIL_BC;
  const int t0 = (int)((int64_t)tiles * blockIdx.y / gridDim.y), t1 = (int)((int64_t)tiles * (blockIdx.y + 1) / gridDim.y);
  const int nk = (Dp + SLIC_RT_BK - 1) / SLIC_RT_BK;
  const int nkp = (nk + SIL_ST - 1) / SIL_ST * SIL_ST;        // a tile is a whole number of ring turns (the extra k-tiles are zeros)
  const SlicRtLane ln = slic_rt_lane(tid, Dp);
  const int xrows = (N - pblock) < SIL_BP ? (N - pblock) : SIL_BP;
  const __amdgpu_buffer_rsrc_t rs_x =
      __builtin_amdgcn_make_buffer_rsrc((void*)(xp + (int64_t)pblock * Dp), 0, xrows * Dp * 4, 0x00020000);
  unsigned xoff[SIL_BP / 32], coff[SIL_NCT];
  slic_rt_offsets(xoff, ln, (unsigned)Dp * 4u, xrows);
  slic_rt_offsets(coff, ln, (unsigned)Dp * 4u);
  auto issue = [&](int tile, int kt, int stage) {
    float* Xs = sil_lds + stage * STAGE_FLOATS;
    const bool tl = tile < t1;
    const bool live = tl && ln.kin(kt);
    const int crows = tl ? ((U - tile * SIL_BC) < SIL_BC ? (U - tile * SIL_BC) : SIL_BC) : 0;
    const __amdgpu_buffer_rsrc_t rs_c =
        __builtin_amdgcn_make_buffer_rsrc((void*)(mp + (tl ? (int64_t)tile * SIL_BC * Dp : 0)), 0, crows * Dp * 4, 0x00020000);
    slic_rt_issue<true>(rs_x, Xs, wave, xoff, 0u, kt, live);
    slic_rt_issue<true>(rs_c, Xs + SIL_BP * SLIC_RT_BK, wave, coff, 0u, kt, live);
  };
  const int p = pblock + 32 * wave + r;
  int myid = p < N ? ids[p] : -1;
  if (myid == ig) myid = -1;
  const float xn = p < N ? xnf[p] : 0.f;
  float own = -1.0f, best = INFINITY;
  int bidx = 0x7fffffff;
  f32x16 acc[SIL_NCT];
  issue(t0, 0, 0);
  for (int tile = t0; tile < t1; ++tile) {
#pragma unroll
    for (int ct = 0; ct < SIL_NCT; ++ct)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[ct][g] = 0.f;
    for (int kt0 = 0; kt0 < nkp; kt0 += SIL_ST) {
#pragma unroll
      for (int sidx = 0; sidx < SIL_ST; ++sidx) {
        slic_rt_wait<(SIL_ST - 2) * PER_STAGE>();
        __builtin_amdgcn_s_barrier();
        const int kn = kt0 + sidx + SIL_ST - 1;
        issue(kn >= nkp ? tile + 1 : tile, kn >= nkp ? kn - nkp : kn, (sidx + SIL_ST - 1) % SIL_ST);
        const float* Xs = sil_lds + sidx * STAGE_FLOATS;
        slic_rt_compute_stage<SIL_NCT>(acc, Xs, Xs + SIL_BP * SLIC_RT_BK, 0, 32 * wave, r, h);
      }
    }
    // the lane's cluster index rises with (tile, ct, g): a strict '<' alone keeps the first minimum
    const int cb = tile * SIL_BC;
#pragma unroll
    for (int ct = 0; ct < SIL_NCT; ++ct)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int c = cb + ct * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        const float d = fmaxf(fmaf(-alpha, acc[ct][g], xn + colq[c]), 0.f);       // colq is padded past U with +inf
        if (c == myid) own = d;
        else if (d < best) { best = d; bidx = c; }
      }
  }
  slic_rt_wait<0>();                                           // the trailing all-zero DMAs must land before the workgroup leaves
  const float oo = __shfl_xor(own, 32);
  const float ob = __shfl_xor(best, 32);
  const int oi = __shfl_xor(bidx, 32);
  own = fmaxf(own, oo);
  if (ob < best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
  if (h == 0 && p < N) {
    const int64_t at = (int64_t)blockIdx.y * N + p;
    pown[at] = own;
    pbest[at] = best;
    pidx[at] = bidx;
  }
}

__global__ __launch_bounds__(SIL_T) void sil_finish(const float* __restrict__ pown, const float* __restrict__ pbest,
                                                   const int* __restrict__ pidx, int G, int N, const int* __restrict__ ids,
                                                   const int* __restrict__ cnt, const uint32_t* __restrict__ uniq,
                                                   const float* __restrict__ selft, const int* __restrict__ meta, float* __restrict__ sbuf,
                                                   float* __restrict__ out_s, float* __restrict__ out_a, float* __restrict__ out_b,
                                                   int32_t* __restrict__ out_nearest) {
  const int i = blockIdx.x * SIL_T + threadIdx.x;
  if (i >= N) return;
  float s = NAN, a = NAN, b = NAN;
  int32_t nearest = 0;
  const int id = ids[i];
  if (!meta[SIL_STATUS] && id == meta[SIL_IG]) nearest = (int32_t)(uniq[id] ^ 0x80000000u);      // an ignored row keeps its own label
  if (!meta[SIL_STATUS] && id != meta[SIL_IG]) {
    float own = pown[i], best = pbest[i];
    int bidx = pidx[i];
    for (int g = 1; g < G; ++g) {
      own = fmaxf(own, pown[(int64_t)g * N + i]);
      const float v = pbest[(int64_t)g * N + i];
      if (v < best) { best = v; bidx = pidx[(int64_t)g * N + i]; }
    }
    const int n = cnt[id];
    b = best;
    if (bidx >= 0 && bidx < meta[SIL_U]) nearest = (int32_t)(uniq[bidx] ^ 0x80000000u);
    if (n <= 1) {
      a = 0.f;
      s = 0.f;
    } else {
      // the row itself leaves the own-cluster total as the term it entered with: n * d_own - (1 - x^.x^)
      const float tot = fmaxf(fmaf((float)n, own, -selft[i]), 0.f);
      a = tot / (float)(n - 1);
      const float m = fmaxf(a, b);
      s = m == 0.f ? 0.f : (b - a) / m;
    }
  }
  sbuf[i] = s;
  if (out_s) out_s[i] = s;
  if (out_a) out_a[i] = a;
  if (out_b) out_b[i] = b;
  if (out_nearest) out_nearest[i] = nearest;
}

// slot j of the per-cluster outputs: the j-th scored cluster by ascending label (the ignored label takes no slot); slots past K: NaN, 0
__global__ __launch_bounds__(SIL_T) void sil_cluster_means(const float* __restrict__ sbuf, const int* __restrict__ ord,
                                                          const int* __restrict__ start, const int* __restrict__ cnt,
                                                          const uint32_t* __restrict__ uniq, const int* __restrict__ meta, int kmax,
                                                          double* __restrict__ cluster_mean, int32_t* __restrict__ cluster_label) {
  __shared__ double sh[SIL_T];
  const int u = blockIdx.x;
  const int U = meta[SIL_U], ig = meta[SIL_IG];
  const bool ok = !meta[SIL_STATUS];
  if (!ok || u >= U) {
    const int j = ok ? u - (ig >= 0 ? 1 : 0) : u;
    if (threadIdx.x == 0 && j >= 0 && j < kmax && (ok || u < kmax)) {
      if (cluster_mean) cluster_mean[j] = NAN;
      if (cluster_label) cluster_label[j] = 0;
    }
    return;
  }
  if (u == ig) return;
  const int n = cnt[u];
  const int* o = ord + start[u];
  double acc = 0.0;
  for (int m = threadIdx.x; m < n; m += SIL_T) acc += (double)sbuf[o[m]];
  const double tot = slic_wg_fold<SIL_T>(acc, sh);
  const int j = u - (ig >= 0 && u > ig ? 1 : 0);
  if (threadIdx.x == 0 && j < kmax) {
    if (cluster_mean) cluster_mean[j] = tot / (double)n;
    if (cluster_label) cluster_label[j] = (int32_t)(uniq[u] ^ 0x80000000u);
  }
}

__global__ __launch_bounds__(SIL_T) void sil_sum_part(const float* __restrict__ sbuf, const int* __restrict__ ids, int N,
                                                     const int* __restrict__ meta, double* __restrict__ part) {
  __shared__ double sh[SIL_T];
  double acc = 0.0;
  if (!meta[SIL_STATUS]) {
    const int ig = meta[SIL_IG];
    for (int i = blockIdx.x * SIL_T + threadIdx.x; i < N; i += SIL_G * SIL_T)
      if (ids[i] != ig) acc += (double)sbuf[i];
  }
  const double r = slic_wg_fold<SIL_T>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(SIL_T) void sil_record(const double* __restrict__ part, const int* __restrict__ meta, double* __restrict__ record) {
  __shared__ double sh[SIL_T];
  const int t = threadIdx.x;
  const double sum = slic_wg_fold<SIL_T>(((part[t] + part[t + SIL_T]) + part[t + 2 * SIL_T]) + part[t + 3 * SIL_T], sh);
  if (t != 0) return;
  const int status = meta[SIL_STATUS];
  record[0] = status ? (double)NAN : sum / (double)meta[SIL_NEFF];
  record[1] = (double)meta[SIL_K];
  record[2] = (double)meta[SIL_NEFF];
  record[3] = (double)status;
}

struct SilLayout {
  SlicLabelScratch ids;
  int *id, *cnt, *meta, *pidx;
  float *xp, *mp, *colq, *xnf, *selft, *sbuf, *pown, *pbest;
  double *xn64, *part;
};

static int sil_dp(int D) { return (D + 7) / 8 * 8; }
static int64_t sil_kcap(int64_t N, int64_t Kmax) { return Kmax + 1 < N ? Kmax + 1 : N; }     // + the ignored label's class
static int64_t sil_colq_len(int64_t kcap) { return slic_cdiv(kcap, SIL_BC) * SIL_BC + SIL_BC; }

static bool sil_size_ok(int64_t N, int D, int64_t Kmax) {
  return N >= 3 && N <= SLIC_SILHOUETTE_MAX_N && D >= 1 && D <= SLIC_SILHOUETTE_MAX_D && Kmax >= 2 && Kmax <= N - 1;
}

static size_t sil_layout(void* base, int64_t N, int D, int64_t Kmax, SilLayout* L) {
  SlicCarver c(base);
  const size_t n = (size_t)N, dp = (size_t)sil_dp(D), kcap = (size_t)sil_kcap(N, Kmax);
  SilLayout l;
  slic_label_scratch_take(c, N, true, &l.ids);
  l.id = c.take<int>(n);
  l.cnt = c.take<int>(n);
  l.meta = c.take<int>(SIL_NMETA);
  l.pidx = c.take<int>(SIL_MAX_SPLIT * n);
  l.xp = c.take<float>(n * dp);
  l.mp = c.take<float>(kcap * dp);
  l.colq = c.take<float>((size_t)sil_colq_len((int64_t)kcap));
  l.xnf = c.take<float>(n);
  l.selft = c.take<float>(n);
  l.sbuf = c.take<float>(n);
  l.pown = c.take<float>(SIL_MAX_SPLIT * n);
  l.pbest = c.take<float>(SIL_MAX_SPLIT * n);
  l.xn64 = c.take<double>(n);
  l.part = c.take<double>(SIL_G);
  if (L) *L = l;
  return c.off;
}

extern "C" size_t slic_silhouette_workspace_bytes(int64_t N, int D, int64_t Kmax) {
  if (!sil_size_ok(N, D, Kmax)) return 0;
  return sil_layout(nullptr, N, D, Kmax, nullptr);
}

extern "C" int slic_silhouette(const float* X, int64_t N, int D, int64_t ldx, const int32_t* labels, int metric, int has_ignore,
                               int32_t ignore_label, int64_t Kmax, float* out_s, float* out_a, float* out_b, int32_t* out_nearest,
                               double* record, double* cluster_mean, int32_t* cluster_label, void* workspace, void* stream) {
  SLIC_REQUIRE(sil_size_ok(N, D, Kmax), "slic_silhouette: N = %lld, D = %d, Kmax = %lld (3 <= N <= %lld, 1 <= D <= %d, 2 <= Kmax <= N - 1)",
               (long long)N, D, (long long)Kmax, (long long)SLIC_SILHOUETTE_MAX_N, SLIC_SILHOUETTE_MAX_D);
  SLIC_REQUIRE(metric == SLIC_SILHOUETTE_COSINE || metric == SLIC_SILHOUETTE_SQEUCLIDEAN, "slic_silhouette: metric %d", metric);
  SLIC_REQUIRE(X && labels && record && workspace && ldx >= D, "slic_silhouette: NULL argument or ldx < D");
  hipStream_t st = S_(stream);
  const int n = (int)N, dp = sil_dp(D), kcap = (int)sil_kcap(N, Kmax), cosine = metric == SLIC_SILHOUETTE_COSINE;
  SilLayout L;
  sil_layout(workspace, N, D, Kmax, &L);
  const int cus = slic_device_cus();
  if (!cus) {
    slic_set_error("slic_silhouette: cannot query the device's compute units");
    return SLIC_EHIP;
  }
  int rc = slic_label_dense_ids(labels, n, L.ids, L.id, L.cnt, L.meta + SIL_U, st);
  if (rc != SLIC_OK) return rc;
  sil_check<<<1, 64, 0, st>>>(L.ids.uniq, L.cnt, n, has_ignore, ignore_label, kcap, (int)Kmax, L.meta);
  SLIC_LAUNCH_CHECK();
  const dim3 gn((unsigned)slic_cdiv(n, SIL_T));
  sil_prep<<<gn, SIL_T, 0, st>>>(X, n, D, ldx, dp, cosine, L.xp, L.xnf, L.selft, L.xn64);
  SLIC_LAUNCH_CHECK();
  const int64_t nq = sil_colq_len(kcap);
  sil_fill<<<(unsigned)slic_cdiv(nq, SIL_T), SIL_T, 0, st>>>(L.colq, nq, INFINITY);
  SLIC_LAUNCH_CHECK();
  sil_stats<<<dim3((unsigned)kcap, (unsigned)slic_cdiv(dp + 1, 64)), 64, 0, st>>>(L.xp, L.xn64, dp, cosine, L.ids.ord_a, L.ids.start, L.cnt,
                                                                                  L.meta, L.mp, L.colq);
  SLIC_LAUNCH_CHECK();
  // the K-group split: enough workgroups for two per compute unit, at most one share per cluster tile the bound admits
  const int64_t row_tiles = slic_cdiv(n, SIL_BP), col_tiles = slic_cdiv(kcap, SIL_BC);
  int split = (int)slic_cdiv(2 * (int64_t)cus, row_tiles);
  if (split > SIL_MAX_SPLIT) split = SIL_MAX_SPLIT;
  if (split > col_tiles) split = (int)col_tiles;
  if (split < 1) split = 1;
  const size_t lds = (size_t)SIL_ST * (SIL_BP + SIL_BC) * SLIC_RT_BK * sizeof(float);
  SLIC_LDS_LIMIT(sil_score, lds);
  sil_score<<<dim3((unsigned)row_tiles, (unsigned)split), 256, lds, st>>>(L.xp, n, dp, L.mp, L.colq, L.xnf, L.id, L.meta,
                                                                          cosine ? 1.0f : 2.0f, L.pown, L.pbest, L.pidx);
  SLIC_LAUNCH_CHECK();
  sil_finish<<<gn, SIL_T, 0, st>>>(L.pown, L.pbest, L.pidx, split, n, L.id, L.cnt, L.ids.uniq, L.selft, L.meta, L.sbuf, out_s, out_a, out_b,
                                   out_nearest);
  SLIC_LAUNCH_CHECK();
  if (cluster_mean || cluster_label) {
    sil_cluster_means<<<(unsigned)kcap, SIL_T, 0, st>>>(L.sbuf, L.ids.ord_a, L.ids.start, L.cnt, L.ids.uniq, L.meta, (int)Kmax, cluster_mean,
                                                        cluster_label);
    SLIC_LAUNCH_CHECK();
  }
  sil_sum_part<<<SIL_G, SIL_T, 0, st>>>(L.sbuf, L.id, n, L.meta, L.part);
  SLIC_LAUNCH_CHECK();
  sil_record<<<1, SIL_T, 0, st>>>(L.part, L.meta, record);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
