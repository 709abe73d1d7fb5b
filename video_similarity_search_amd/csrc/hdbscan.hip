// HDBSCAN with the cosine metric: the O(N^2 D) part of sklearn.cluster.HDBSCAN(min_cluster_size, min_samples, metric='cosine') on the device.
//
// The contract is in include/slic_hip.h (slic_hdbscan_core); in short d(i, j) = clip(1 - x_i.x_j, 0, 2) on unit rows, core(i) = the
// min_samples-th smallest entry of row i of d with the diagonal zero counted, w(i, j) = max(d(i, j), core(i), core(j)), and the tree is
// the minimum spanning tree of w under the total order (w, min(i, j), max(i, j)).  The tree is built by Boruvka rounds: the host keeps
// the components (clustering/hdbscan.py), the device finds every component's lightest edge to a foreign row.
//
// Passes (on the normalised, zero-padded rows Xn [N, Dp], Dp = D rounded up to 8, kept in the workspace between the calls):
//   prep     inv[i] in float64, Xn[i] = fp32(x_i * inv[i])                                                        (slic_hdbscan_core)
//   core     slic_cosine_topk of Xn against itself, self_mask = 0, k = min_samples; one wave per row then recomputes the distance to
//            the list's last row in float64 from the raw rows (hd_d64: a fixed summation order, symmetric in the pair)
//   round    hd_tiles: the similarity GEMM over ALL 128 x 128 tiles (every row needs its own minimum), the matrix loop of db_tiles:
//            query operand in registers, gallery tiles through the 4-stage DMA ring of mfma_ring.h, v_mfma_f32_32x32x2_f32.  Epilogue on
//            each accumulator block: d from the score, max with the two core distances, rows of the query's own component masked, a
//            running (w, j) per lane (gallery rows ascend inside a lane, so a strict < keeps the smaller j).  The two lane halves and
//            the gallery slices meet in one 64-bit atomicMin per row on (w bits << 32 | j): integer, order-independent.
//            hd_comp_min / hd_comp_hi / hd_emit: the least (w, lo, hi) of every component's rows, again by integer atomicMin.
//   weights  hd_pair_w: float64 w for a list of pairs, one wave per pair                                          (slic_hdbscan_edge_weights)
// No float atomics anywhere: two runs are bit-equal.  The N x N matrix is never written.
#include "mfma_ring.h"
#include "dbscan_shared.h"
#include <math.h>
#include <limits.h>
#include <stdlib.h>
#include <algorithm>

#define HD_SLICE 16           // gallery tiles per workgroup
#define HD_KMAX 88            // slic_cosine_topk's list limit: min_samples
#define HD_NONE 0xFFFFFFFFFFFFFFFFull

typedef unsigned long long u64;

// d of rule 1 in float64 for one pair, by one wave: lane l takes elements l, l + 64, ... of the raw rows (lower row first) by fma, then
// an xor butterfly; every lane returns the value.  The order is fixed and the same from either end of the pair.
__device__ __forceinline__ double hd_d64(const float* __restrict__ X, int ldx, int D, const double* __restrict__ inv, int i, int j, int lane) {
  if (i == j) return 0.0;
  const int a = min(i, j), b = max(i, j);
  const float* xa = X + (int64_t)a * ldx;
  const float* xb = X + (int64_t)b * ldx;
  double s = 0.0;
  for (int k = lane; k < D; k += 64) s = fma((double)xa[k], (double)xb[k], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const double d = 1.0 - s * inv[a] * inv[b];
  return fmin(fmax(d, 0.0), 2.0);
}

// core distances: one wave per row; knn: [N, k] lists of slic_cosine_topk with the row itself in them
__global__ __launch_bounds__(256) void hd_core(const float* __restrict__ X, int N, int ldx, int D, const double* __restrict__ inv,
                                               const int32_t* __restrict__ knn, int k, double* __restrict__ core, float* __restrict__ core32) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  int j = knn[(int64_t)row * k + k - 1];
  if (j < 0 || j >= N || k == 1) j = row;                      // min_samples = 1: the diagonal zero itself (a zero row scores 0, not 1, against itself)
  const double c = hd_d64(X, ldx, D, inv, row, j, lane);
  if (lane == 0) { core[row] = c; core32[row] = (float)c; }
}

// float64 w of rule 3 for M pairs: one wave per pair
__global__ __launch_bounds__(256) void hd_pair_w(const float* __restrict__ X, int N, int ldx, int D, const double* __restrict__ inv,
                                                 const double* __restrict__ core, const int32_t* __restrict__ pairs, int64_t M,
                                                 double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= M) return;
  const int i = pairs[2 * e], j = pairs[2 * e + 1];
  double w = __longlong_as_double(0x7ff8000000000000ll);      // a pair outside the rows: NaN
  if (i >= 0 && i < N && j >= 0 && j < N) w = fmax(hd_d64(X, ldx, D, inv, i, j, lane), fmax(core[i], core[j]));
  if (lane == 0) out[e] = w;
}

struct HdArgs {
  const float* Xn;           // [N, Dp]
  int N, Dp;
  const float* core;         // [N] fp32 core distances
  const int* comp;           // [N] component of every row
  u64* rowbest;              // [N] (w bits << 32) | j, HD_NONE = no foreign row
};

// one workgroup = one 128-row query tile (A, in registers) x a slice of up to HD_SLICE gallery tiles (B, through the DMA ring)
template <int NK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void hd_tiles(HdArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(NK % 4 == 0, "a gallery tile is a whole number of ring turns");
  float* gcore = lds + 4 * SLIC_RT_TILE;                       // [128] core distances of the gallery tile (+inf past the rows)
  int* gcomp = (int*)(gcore + DB_B);                           // [128] components of the gallery tile
  const int N = p.N, Dp = p.Dp;
  const int I = blockIdx.x;
  const int nbt = (N + DB_B - 1) / DB_B;
  const int jbeg = blockIdx.y * HD_SLICE;
  const int ntl = min(jbeg + HD_SLICE, nbt) - jbeg;
  if (I * DB_B >= N || ntl <= 0) return;                       // (workgroup-uniform, before any barrier)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  const int q = I * DB_B + 32 * wave + r;
  const bool qvalid = q < N;
  const int qs = qvalid ? q : N - 1;
  f32x4 qr[NK][4];
  slic_rt_load_frags<NK>(qr, p.Xn + (int64_t)qs * Dp, Dp, h);
  const float cq = p.core[qs];
  const int compq = p.comp[qs];

  const SlicRtLane ln = slic_rt_lane(tid, Dp);
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)p.Xn, 0, (int)((int64_t)N * Dp * 4), 0x00020000);
  unsigned goff[4];
  slic_rt_offsets<4>(goff, ln, (unsigned)Dp * 4u);
  // ring step (tile, kt) into `stage`; a tile past the slice and a k-tile past Dp come from out of range: zeros
  auto issue = [&](int tile, int kt, int stage) {
    const unsigned gb = tile < ntl ? (unsigned)(jbeg + tile) * (unsigned)(DB_B * Dp * 4) : 0u;
    slic_rt_issue(rs_g, lds + stage * SLIC_RT_TILE, wave, goff, gb, kt, ln.kin(kt) && tile < ntl);
  };

  float bw = INFINITY;                                         // this lane's lightest foreign row so far
  int bj = -1;
  f32x16 acc[4];
  f32x4 a[2][4];
  float ncore = INFINITY;                                      // this thread's gallery row of the next tile (tid < 128)
  int ncomp = -1;
  issue(0, 0, 0);
  issue(0, 1, 1);
  issue(0, 2, 2);
  slic_rt_wait<8>();                                           // step 0 has landed
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) a[0][ct] = *(const f32x4*)&lds[slic_rt_off(32 * ct + r, h)];
  for (int tile = 0; tile < ntl; ++tile) {
    const int g0 = (jbeg + tile) * DB_B;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ct][v] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
      slic_rt_wait<4>();                                       // step s + 1 has landed (this wave's part of it)
      __builtin_amdgcn_s_barrier();                            // ... everybody's; and stage (kt + 3) & 3 has been read by all
      {
        const int kn = kt + 3;
        issue(kn >= NK ? tile + 1 : tile, kn >= NK ? kn - NK : kn, kn & 3);
      }
      // the previous tile's epilogue is over (barrier of kt = 0): the gallery rows' core distances and components, published at
      // kt = 2 and visible after the barrier of kt = 3
      if (kt == 0) {
        if (tid < DB_B) {
          const bool in = g0 + tid < N;
          ncore = in ? p.core[g0 + tid] : INFINITY;
          ncomp = in ? p.comp[g0 + tid] : -1;
        }
      } else if (kt == 2) {
        if (tid < DB_B) { gcore[tid] = ncore; gcomp[tid] = ncomp; }
      }
      slic_rt_ktile_mfma<false, 4>(acc, a, qr[kt], lds, kt & 3, r, h);
    }
    // ---- epilogue: lane (r, h) holds query q against gallery rows g0 + ct * 32 + (v & 3) + 8 (v >> 2) + 4 h, ascending in (ct, v).
    // A row past N has core = +inf: its w is never < bw.  A zero row scores 0 against everything: d = 1 (rule 1).
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int v4 = 0; v4 < 4; ++v4) {
        const int gl = ct * 32 + 8 * v4 + 4 * h;
        const f32x4 gc = *(const f32x4*)&gcore[gl];
        const i32x4 gm = *(const i32x4*)&gcomp[gl];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = fminf(fmaxf(1.f - acc[ct][4 * v4 + e], 0.f), 2.f);
          const float w = fmaxf(fmaxf(d, cq), gc[e]);
          if (gm[e] != compq && w < bw) { bw = w; bj = g0 + gl + e; }
        }
      }
  }
  {
    const float ow = __shfl_xor(bw, 32);
    const int oj = __shfl_xor(bj, 32);
    // w >= 0: the bits of a float order as the unsigned integer does
    u64 key = bj >= 0 ? ((u64)__float_as_uint(bw) << 32) | (unsigned)bj : HD_NONE;
    const u64 okey = oj >= 0 ? ((u64)__float_as_uint(ow) << 32) | (unsigned)oj : HD_NONE;
    key = okey < key ? okey : key;
    if (h == 0 && qvalid && key != HD_NONE) atomicMin(&p.rowbest[q], key);
  }
  slic_rt_wait<0>();                                           // the trailing all-zero DMAs must land before the workgroup leaves
}

// the least (w, lo) of every component's rows, lo = min(i, j)
__global__ __launch_bounds__(256) void hd_comp_min(const u64* __restrict__ rowbest, const int* __restrict__ comp, int N, int C,
                                                   u64* __restrict__ cbest) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const u64 key = rowbest[i];
    const int c = comp[i];
    if (key == HD_NONE || (unsigned)c >= (unsigned)C) continue;
    const int j = (int)(unsigned)(key & 0xFFFFFFFFull);
    atomicMin(&cbest[c], (key & 0xFFFFFFFF00000000ull) | (unsigned)min(i, j));
  }
}

// ... and among the rows that reach it the least hi = max(i, j): the component's candidate is its least (w, lo, hi), rule 4's order
__global__ __launch_bounds__(256) void hd_comp_hi(const u64* __restrict__ rowbest, const int* __restrict__ comp, int N, int C,
                                                  const u64* __restrict__ cbest, int* __restrict__ chi) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const u64 key = rowbest[i];
    const int c = comp[i];
    if (key == HD_NONE || (unsigned)c >= (unsigned)C) continue;
    const int j = (int)(unsigned)(key & 0xFFFFFFFFull);
    if (((key & 0xFFFFFFFF00000000ull) | (unsigned)min(i, j)) == cbest[c]) atomicMin(&chi[c], max(i, j));
  }
}

__global__ __launch_bounds__(256) void hd_emit(const u64* __restrict__ cbest, const int* __restrict__ chi, int C, int32_t* __restrict__ out_i,
                                               int32_t* __restrict__ out_j, float* __restrict__ out_w) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x) {
    const u64 key = cbest[c];
    const bool none = key == HD_NONE;
    out_i[c] = none ? -1 : (int)(unsigned)(key & 0xFFFFFFFFull);
    out_j[c] = none ? -1 : chi[c];
    out_w[c] = none ? INFINITY : __uint_as_float((unsigned)(key >> 32));
  }
}

// ------------------------------------------------------------------------------------------------------------------------------

struct HdLayout {
  u64* stats; int* meta; double* inv; float* Xn; float* core32; int32_t* knn; float* knn_dist; char* topk_ws;
  u64* rowbest; u64* cbest; int* chi;
};

static size_t hd_layout(void* base, int64_t N, int Dp, int k, HdLayout* L) {
  SlicCarver c(base);
  HdLayout l;
  l.stats = c.take<u64>(8);
  l.meta = c.take<int>(8);                                     // [0] N, [1] D, [2] min_samples of the slic_hdbscan_core call
  l.inv = c.take<double>(N);
  l.Xn = c.take<float>((size_t)N * Dp);
  l.core32 = c.take<float>(N);
  l.knn = c.take<int32_t>((size_t)N * k);
  l.knn_dist = c.take<float>((size_t)N * k);
  l.topk_ws = c.take<char>(slic_cosine_topk_workspace_bytes((int)N, (int)N, k));
  l.rowbest = c.take<u64>(N);
  l.cbest = c.take<u64>(N);
  l.chi = c.take<int>(N);
  if (L) *L = l;
  return c.off;
}

static bool hd_args_ok(int64_t N, int D, int min_samples) {
  return N >= 2 && db_size_ok(N, D) && min_samples >= 1 && min_samples <= N && min_samples <= HD_KMAX;
}

extern "C" size_t slic_hdbscan_workspace_bytes(int64_t N, int D, int min_samples) {
  if (!hd_args_ok(N, D, min_samples)) return 0;
  return hd_layout(nullptr, N, (D + 7) / 8 * 8, min_samples, nullptr);
}

// the host-side record for slic_hdbscan_stats: counts since the last slic_hdbscan_core, times when SLIC_HDBSCAN_TIMING=1
enum { HD_EV_CORE0, HD_EV_CORE1, HD_EV_ROUND0, HD_EV_PASS1, HD_EV_ROUND1, HD_NEV };
static hipEvent_t hd_ev[HD_NEV];
static struct { bool timed; int rounds; int64_t rows_last; double ms_core, ms_rounds, ms_last_round, ms_last_pass; } hd_last;

static int hd_timing(void) {
  const char* tenv = getenv("SLIC_HDBSCAN_TIMING");
  hd_last.timed = tenv && tenv[0] == '1';
  if (hd_last.timed)
    for (int i = 0; i < HD_NEV; ++i)
      if (!hd_ev[i]) SLIC_HIP_CHECK(hipEventCreate(&hd_ev[i]));
  return SLIC_OK;
}

extern "C" int slic_hdbscan_core(const float* X, int64_t N, int ldx, int D, int min_samples, double* core_dist, void* workspace,
                                 void* stream) {
  SLIC_REQUIRE(D >= 1 && D <= 512, "slic_hdbscan_core: D = %d (1 <= D <= 512)", D);
  SLIC_REQUIRE(N >= 2 && db_size_ok(N, D), "slic_hdbscan_core: N = %lld rows of D = %d (2 <= N, int32 row indices, N x Dp x 4 bytes < 4 GiB)",
               (long long)N, D);
  SLIC_REQUIRE(min_samples >= 1 && min_samples <= N, "slic_hdbscan_core: min_samples = %d (1 <= min_samples <= N = %lld)", min_samples,
               (long long)N);
  SLIC_REQUIRE(min_samples <= HD_KMAX, "slic_hdbscan_core: min_samples = %d (the core-distance search keeps lists of at most %d rows)",
               min_samples, HD_KMAX);
  SLIC_REQUIRE(ldx >= D, "slic_hdbscan_core: ldx = %d < D = %d", ldx, D);
  SLIC_REQUIRE(X && core_dist && workspace, "slic_hdbscan_core: NULL argument");
  hipStream_t st = S_(stream);
  const int n = (int)N;
  const int Dp = (D + 7) / 8 * 8;
  const int k = min_samples;
  HdLayout L;
  hd_layout(workspace, N, Dp, k, &L);
  { int r = hd_timing(); if (r) return r; }
  hd_last.rounds = 0; hd_last.rows_last = 0;
  hd_last.ms_core = hd_last.ms_rounds = hd_last.ms_last_round = hd_last.ms_last_pass = -1.0;
  if (hd_last.timed) SLIC_HIP_CHECK(hipEventRecord(hd_ev[HD_EV_CORE0], st));
  const int meta[3] = {n, D, min_samples};
  SLIC_HIP_CHECK(hipMemcpyAsync(L.meta, meta, sizeof(meta), hipMemcpyHostToDevice, st));
  db_prep<0><<<(n + 3) / 4, 256, 0, st>>>(X, n, ldx, D, Dp, L.inv, L.Xn);
  SLIC_LAUNCH_CHECK();
  { int r = slic_cosine_topk(L.Xn, n, L.Xn, n, Dp, k, 0, L.knn, L.knn_dist, L.topk_ws, stream); if (r) return r; }
  hd_core<<<(n + 3) / 4, 256, 0, st>>>(X, n, ldx, D, L.inv, L.knn, k, core_dist, L.core32);
  SLIC_LAUNCH_CHECK();
  if (hd_last.timed) {
    float ms = -1.f;
    SLIC_HIP_CHECK(hipEventRecord(hd_ev[HD_EV_CORE1], st));
    SLIC_HIP_CHECK(hipEventSynchronize(hd_ev[HD_EV_CORE1]));
    SLIC_HIP_CHECK(hipEventElapsedTime(&ms, hd_ev[HD_EV_CORE0], hd_ev[HD_EV_CORE1]));
    hd_last.ms_core = ms;
    hd_last.ms_rounds = 0.0;
  }
  return SLIC_OK;
}

static int hd_launch_tiles(int NK, dim3 grid, size_t lds, hipStream_t st, const HdArgs& a) {
  const auto kern = NK == 4 ? hd_tiles<4> : NK == 8 ? hd_tiles<8> : NK == 12 ? hd_tiles<12> : hd_tiles<16>;
  SLIC_LDS_LIMIT(kern, lds);
  kern<<<grid, dim3(256), lds, st>>>(a);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_hdbscan_round(void* workspace, int64_t N, int D, int min_samples, const int32_t* comp, int C, int32_t* out_i,
                                  int32_t* out_j, float* out_w, uint64_t* row_best, void* stream) {
  SLIC_REQUIRE(hd_args_ok(N, D, min_samples), "slic_hdbscan_round: N = %lld, D = %d, min_samples = %d are outside slic_hdbscan_core's limits",
               (long long)N, D, min_samples);
  SLIC_REQUIRE(C >= 1 && C <= N, "slic_hdbscan_round: C = %d components (1 <= C <= N = %lld)", C, (long long)N);
  SLIC_REQUIRE(workspace && comp && out_i && out_j && out_w, "slic_hdbscan_round: NULL argument");
  hipStream_t st = S_(stream);
  const int n = (int)N;
  const int Dp = (D + 7) / 8 * 8;
  const int NK = (Dp + 127) / 128 * 4;
  HdLayout L;
  hd_layout(workspace, N, Dp, min_samples, &L);
  u64* rowbest = row_best ? (u64*)row_best : L.rowbest;
  { int r = hd_timing(); if (r) return r; }
  if (hd_last.timed) SLIC_HIP_CHECK(hipEventRecord(hd_ev[HD_EV_ROUND0], st));
  SLIC_HIP_CHECK(hipMemsetAsync(rowbest, 0xFF, (size_t)n * sizeof(u64), st));
  SLIC_HIP_CHECK(hipMemsetAsync(L.cbest, 0xFF, (size_t)C * sizeof(u64), st));
  SLIC_HIP_CHECK(hipMemsetAsync(L.chi, 0x7F, (size_t)C * sizeof(int), st));
  HdArgs a;
  a.Xn = L.Xn; a.N = n; a.Dp = Dp; a.core = L.core32; a.comp = comp; a.rowbest = rowbest;
  const int T = (n + DB_B - 1) / DB_B;
  const dim3 grid(T, (T + HD_SLICE - 1) / HD_SLICE);
  constexpr size_t LDS = 4 * SLIC_RT_TILE * 4 + 2 * DB_B * 4;
  { int r = hd_launch_tiles(NK, grid, LDS, st, a); if (r) return r; }
  if (hd_last.timed) SLIC_HIP_CHECK(hipEventRecord(hd_ev[HD_EV_PASS1], st));
  const int gn = (int)std::min<int64_t>(4096, slic_cdiv(n, 256));
  hd_comp_min<<<gn, 256, 0, st>>>(rowbest, comp, n, C, L.cbest);
  SLIC_LAUNCH_CHECK();
  hd_comp_hi<<<gn, 256, 0, st>>>(rowbest, comp, n, C, L.cbest, L.chi);
  SLIC_LAUNCH_CHECK();
  hd_emit<<<(int)std::min<int64_t>(4096, slic_cdiv(C, 256)), 256, 0, st>>>(L.cbest, L.chi, C, out_i, out_j, out_w);
  SLIC_LAUNCH_CHECK();
  hd_last.rounds += 1;
  hd_last.rows_last = N;
  if (hd_last.timed) {
    float ms = -1.f, msp = -1.f;
    SLIC_HIP_CHECK(hipEventRecord(hd_ev[HD_EV_ROUND1], st));
    SLIC_HIP_CHECK(hipEventSynchronize(hd_ev[HD_EV_ROUND1]));
    SLIC_HIP_CHECK(hipEventElapsedTime(&ms, hd_ev[HD_EV_ROUND0], hd_ev[HD_EV_ROUND1]));
    SLIC_HIP_CHECK(hipEventElapsedTime(&msp, hd_ev[HD_EV_ROUND0], hd_ev[HD_EV_PASS1]));
    hd_last.ms_last_round = ms;
    hd_last.ms_last_pass = msp;
    hd_last.ms_rounds = (hd_last.ms_rounds < 0.0 ? 0.0 : hd_last.ms_rounds) + ms;
  }
  return SLIC_OK;
}

extern "C" int slic_hdbscan_edge_weights(const float* X, int64_t N, int ldx, int D, int min_samples, const double* core_dist,
                                         const int32_t* pairs, int64_t M, double* out, void* workspace, void* stream) {
  SLIC_REQUIRE(hd_args_ok(N, D, min_samples), "slic_hdbscan_edge_weights: N = %lld, D = %d, min_samples = %d are outside slic_hdbscan_core's "
               "limits", (long long)N, D, min_samples);
  SLIC_REQUIRE(M >= 1 && M <= ((int64_t)1 << 31) - 4, "slic_hdbscan_edge_weights: M = %lld pairs (1 <= M < 2^31)", (long long)M);
  SLIC_REQUIRE(ldx >= D, "slic_hdbscan_edge_weights: ldx = %d < D = %d", ldx, D);
  SLIC_REQUIRE(X && core_dist && pairs && out && workspace, "slic_hdbscan_edge_weights: NULL argument");
  HdLayout L;
  hd_layout(workspace, N, (D + 7) / 8 * 8, min_samples, &L);
  hd_pair_w<<<(unsigned)slic_cdiv(M, 4), 256, 0, S_(stream)>>>(X, (int)N, ldx, D, L.inv, core_dist, pairs, M, out);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_hdbscan_stats(double* out_host) {
  SLIC_REQUIRE(out_host, "slic_hdbscan_stats: NULL argument");
  out_host[0] = hd_last.rounds;
  out_host[1] = (double)hd_last.rows_last;
  out_host[2] = hd_last.ms_core;
  out_host[3] = hd_last.ms_rounds;
  out_host[4] = hd_last.ms_last_round;
  out_host[5] = hd_last.ms_last_pass;
  return SLIC_OK;
}
