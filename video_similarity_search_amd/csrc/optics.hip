// OPTICS with the cosine metric, cluster_method='dbscan' cut at eps = max_eps:
//   sklearn.cluster.OPTICS(min_samples, max_eps, metric='cosine', cluster_method='dbscan').fit(X)
// labels_, core_distances_, reachability_, predecessor_ and ordering_ on the device.  Stands in for the reference's
// clustering/cluster_masks.py:88-89 (sklearn on the host).  The contract is in include/slic_hip.h (slic_optics_cosine, rules 1-6).
//
// Two observations make it parallel:
//   * the labels need no walk: they are DBSCAN's at eps = max_eps with one more test on a border row (its cluster's smallest core row must
//     be below it: otherwise the walk meets the row as a start of its own and it stays noise).  db_label_passes of dbscan.hip computes them.
//   * the walk splits by cluster: while cluster c is walked, the unprocessed neighbours of its core rows are exactly the unprocessed rows
//     labelled c, so every cluster's walk reads and writes its own rows only and all clusters walk at once.  ordering_ is the interleaving
//     by start time: a noise row at time = its index, cluster c's block at time = its smallest row; one prefix scan gives the offsets.
//
// Passes after the labels:
//   core    slic_cosine_topk (self-masked, k = min_samples - 1) on the normalised rows Xn; one wave per core row rescoring the last entry
//           with op_d32, the ONE distance function of the walk.
//   layout  cluster sizes and smallest rows (atomics on integers), the scan of the block sizes in row order, every row placed into its
//           cluster's segment.  The order inside a segment is whatever the placement's atomics gave; nothing below depends on it, because
//           a pick is the minimum of (reachability, row), a total order.
//   walk    two forms.  ONE workgroup walks a cluster start to finish (op_walk_small: reachability, predecessor and the processed flags in
//           LDS, a bounded for loop over its size, pick = workgroup argmin, relax = one wave per row); or the host walks clusters step by
//           step, a pick launch and a relax launch per step over all of them, max |C| steps, state in global memory.  No workgroup ever
//           waits on another inside a kernel.  The host reads the sizes' summary back once (clusters, how many go through the host loop,
//           the largest) to size the grids and the loop: the only synchronisation inside the fit.
//           Which form (profiles/optics.txt, MI355X, 20 000 x 128): a step of a cluster of m rows costs its one workgroup m / 16 dependent
//           wave dots and two barriers, the host loop two launches (9-11 us a step measured, whatever m and however many clusters: the
//           relax spreads over the device).  Both are latency, and on one stream they ADD: with clusters of 20-300 rows the fit took
//           6.30 ms all in LDS, 6.45 ms all through the host loop, 7.96 ms with the 15 clusters above 256 rows in the loop and the rest in
//           LDS, 6.66 ms with only the clusters of <= 64 rows in LDS; with clusters of 300-1000 rows 29.8 ms all in LDS, 21.0 ms split at
//           512, 14.0 ms all through the loop.  The one-workgroup time grows with the square of the largest cluster, the loop's with its
//           size; they meet just above 300 rows.  So the LARGEST cluster decides: at most OP_LDS_DEFAULT rows and every cluster gets its
//           workgroup; beyond, every cluster above OP_LDS_SMALL rows goes through the loop (the small ones keep their workgroups: that
//           costs 0.2 ms and keeps thousands of tiny clusters out of the loop's grids).  SLIC_OPTICS_LDS_ROWS (0 .. OP_LDS_ROWS) replaces
//           OP_LDS_DEFAULT for such a measurement (scripts/bench_optics.py).
#include "dbscan_shared.h"
#include <limits.h>
#include <cmath>
#include <stdlib.h>
#include <algorithm>

#define OP_LDS_ROWS 1024      // rows of walk state op_walk_small has room for (13 KB of LDS)
#define OP_LDS_DEFAULT 320    // largest cluster of a fit whose clusters are all walked by one workgroup each (SLIC_OPTICS_LDS_ROWS overrides)
#define OP_LDS_SMALL 64       // ... and in any other fit the clusters up to this size still are
#define OP_RELAX_WGS 131072   // workgroups of one relax launch, about
#define OP_WG 1024            // threads of op_walk_small and op_pick_large
#define OP_NEV (DB_NEV + 2)
#define OP_KMAX 88            // slic_cosine_topk's list limit: min_samples - 1

// rule 3: the fp32 cosine distance of two normalised zero-padded rows.  Lane l takes elements l, l + 64, ... in that order (explicit fmaf),
// the 64 partial sums meet in an xor butterfly (the lane order of pairdist.h), every lane ends with the same bits.  fmaf(x, y, s) and
// a + b are commutative, so op_d32(a, b) == op_d32(b, a) bit for bit; d(i, i) = 0 is the caller's (by index).
// Error on unit rows against the float64 distance of the raw rows, u = 2^-24: the elements of Xn carry one rounding each (the products 2 u,
// and sum |x_k y_k| <= 1), a partial sum passes through at most ceil(Dp / 64) fmaf and 6 butterfly roundings (adding a zero lane is
// exact, so no more than Dp of them in all), and 1 - s rounds once with |d| <= 2: |d32 - d64| <= (min(Dp, Dp / 64 + 7) + 4) u (1 + O(u))
// <= (Dp + 8) u for every Dp >= 8.
__device__ __forceinline__ float op_d32(const float* __restrict__ a, const float* __restrict__ b, int Dp, int lane) {
  float s = 0.f;
  for (int k = lane; k < Dp; k += 64) s = fmaf(a[k], b[k], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  return fminf(fmaxf(1.0f - s, 0.f), 2.f);
}

struct OpArgs {
  const float* Xn; int Dp;                                       // normalised rows
  const float* X; int ldx, D; const double* inv; double eps;     // the exact path (db_exact)
  double dlo, dhi;             // d32 <= dlo: neighbour; > dhi: not; between: float64 decision
  const uint8_t* is_core; const float* cd;
  const int* csize; const int* segoff; const int* seg_row;
  float* reach; int* pred; int* ordering;                        // outputs, indexed by row (ordering: by position)
  int* done;                   // host loop: processed flag by row
  const int* large; int* cur;  // host loop: cluster list, picked row per list entry
  unsigned long long* stats;   // [2] band rechecks of the walk
  int lds_rows;
};

// r = max(d32(p, j), cd[p]) when j is a neighbour of p under rule 1, else -1; the same value on every lane of the wave
__device__ __forceinline__ float op_reach_from(const OpArgs& a, int p, float cdp, int j, int lane) {
  const float d = op_d32(a.Xn + (int64_t)p * a.Dp, a.Xn + (int64_t)j * a.Dp, a.Dp, lane);
  bool nb;
  if ((double)d <= a.dlo) nb = true;
  else if ((double)d > a.dhi) nb = false;
  else {
    int e = 0;
    if (lane == 0) {
      e = db_exact(a.X, a.ldx, a.D, a.inv, p, j, a.eps) ? 1 : 0;
      atomicAdd(&a.stats[2], 1ull);
    }
    nb = __shfl(e, 0) != 0;
  }
  return nb ? fmaxf(d, cdp) : -1.f;
}

// (reachability, row) of a is before that of b: rule 4's pick order
__device__ __forceinline__ bool op_before(float ra, int ia, float rb, int ib) { return ra < rb || (ra == rb && ia < ib); }

// argmin of (r, row) over the workgroup; pos travels with it.  Threads without a candidate pass row = INT_MAX, r = +inf.
// Returns on every thread; sh: 3 * (OP_WG / 64) words.
__device__ __forceinline__ void op_wg_argmin(float& r, int& row, int& pos, int* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float r2 = __shfl_xor(r, o);
    const int i2 = __shfl_xor(row, o), p2 = __shfl_xor(pos, o);
    if (op_before(r2, i2, r, row)) { r = r2; row = i2; pos = p2; }
  }
  if (lane == 0) { sh[3 * w] = __float_as_int(r); sh[3 * w + 1] = row; sh[3 * w + 2] = pos; }
  __syncthreads();
  r = __int_as_float(sh[0]); row = sh[1]; pos = sh[2];
  for (int i = 1; i < nw; ++i) {
    const float r2 = __int_as_float(sh[3 * i]);
    const int i2 = sh[3 * i + 1];
    if (op_before(r2, i2, r, row)) { r = r2; row = i2; pos = sh[3 * i + 2]; }
  }
  __syncthreads();
}

// core distances: one wave per row; knn: [N, k] lists of slic_cosine_topk, the last entry is the (min_samples - 1)-th nearest other row
__global__ __launch_bounds__(256) void op_core_dist(const float* __restrict__ Xn, int N, int Dp, const uint8_t* __restrict__ is_core,
                                                    const int32_t* __restrict__ knn, int k, float* __restrict__ cd) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float v = INFINITY;
  if (is_core[row]) {
    const int j = knn[(int64_t)row * k + k - 1];
    if (j >= 0 && j < N) v = op_d32(Xn + (int64_t)row * Dp, Xn + (int64_t)j * Dp, Dp, lane);
  }
  if (lane == 0) cd[row] = v;
}

__global__ __launch_bounds__(256) void op_init(int N, float* __restrict__ reach, int* __restrict__ pred, int* __restrict__ csize,
                                               int* __restrict__ cstart, int* __restrict__ cursor, int* __restrict__ done,
                                               int* __restrict__ ometa) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    reach[i] = INFINITY;
    pred[i] = -1;
    csize[i] = 0;
    cstart[i] = INT_MAX;
    cursor[i] = 0;
    done[i] = 0;
    if (i < 8) ometa[i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8 && threadIdx.x >= N) ometa[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void op_sizes(const int32_t* __restrict__ labels, int N, int* __restrict__ csize, int* __restrict__ cstart) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int l = labels[i];
    if (l >= 0) {
      atomicAdd(&csize[l], 1);
      atomicMin(&cstart[l], i);
    }
  }
}

// block offsets of ordering_: row i opens a block of 1 (noise), of csize[c] (the smallest row of cluster c) or of 0 rows; the exclusive scan
// in row order places the blocks.  Noise rows are written to ordering_ here.  Then the summary the host reads: ometa[0] clusters,
// [1] clusters the host loop walks (listed in large[]): none when the largest cluster has at most lds_rows rows, else those above
// min(lds_rows, OP_LDS_SMALL), [2] the largest of those, [3] the largest cluster.
__global__ __launch_bounds__(DB_SCAN_T) void op_offsets(const int32_t* __restrict__ labels, int N, const int* __restrict__ csize,
                                                        const int* __restrict__ cstart, const int32_t* __restrict__ n_clusters, int lds_rows,
                                                        int* __restrict__ segoff, int32_t* __restrict__ ordering, int* __restrict__ large,
                                                        int* __restrict__ ometa) {
  __shared__ int sh[DB_SCAN_T / 64];
  __shared__ int largest;
  int beg, end;
  slic_run_bounds(N, DB_SCAN_T, threadIdx.x, &beg, &end);
  if (threadIdx.x == 0) largest = 0;
  int o[1] = {0}, tot[1];
  for (int i = beg; i < end; ++i) {
    const int l = labels[i];
    o[0] += l < 0 ? 1 : (cstart[l] == i ? csize[l] : 0);
  }
  slic_wg_scan<DB_SCAN_T, 1>(o, sh, tot);
  for (int i = beg; i < end; ++i) {
    const int l = labels[i];
    if (l < 0) ordering[o[0]++] = i;
    else if (cstart[l] == i) { segoff[l] = o[0]; o[0] += csize[l]; }
  }
  const int nc = *n_clusters;
  for (int c = threadIdx.x; c < nc; c += DB_SCAN_T) atomicMax(&largest, csize[c]);      // (after slic_wg_scan's barriers)
  __syncthreads();
  if (largest > lds_rows) {
    const int thr = min(lds_rows, OP_LDS_SMALL);
    for (int c = threadIdx.x; c < nc; c += DB_SCAN_T)
      if (csize[c] > thr) large[atomicAdd(&ometa[1], 1)] = c;           // (ometa was zeroed by op_init)
  }
  if (threadIdx.x == 0) {
    ometa[0] = nc;
    ometa[2] = largest > lds_rows ? largest : 0;
    ometa[3] = largest;
  }
}

__global__ __launch_bounds__(256) void op_place(const int32_t* __restrict__ labels, int N, const int* __restrict__ segoff,
                                                int* __restrict__ cursor, int* __restrict__ seg_row) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int l = labels[i];
    if (l >= 0) seg_row[segoff[l] + atomicAdd(&cursor[l], 1)] = i;
  }
}

// one workgroup walks cluster blockIdx.x from its first pick to its last: m <= lds_rows <= OP_LDS_ROWS steps, state in LDS
__global__ __launch_bounds__(OP_WG) void op_walk_small(OpArgs a) {
  __shared__ float s_reach[OP_LDS_ROWS];
  __shared__ int s_pred[OP_LDS_ROWS];
  __shared__ int s_row[OP_LDS_ROWS];
  __shared__ uint8_t s_done[OP_LDS_ROWS];
  __shared__ int sh[3 * (OP_WG / 64)];
  const int c = blockIdx.x;
  const int m = a.csize[c];
  if (m > a.lds_rows || m > OP_LDS_ROWS || m < 1) return;          // (workgroup-uniform) the host loop walks the others
  const int base = a.segoff[c];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < m; k += OP_WG) {
    s_row[k] = a.seg_row[base + k];
    s_reach[k] = INFINITY;
    s_pred[k] = -1;
    s_done[k] = 0;
  }
  __syncthreads();
  for (int step = 0; step < m; ++step) {
    float r = INFINITY;
    int row = INT_MAX, pos = -1;
    for (int k = tid; k < m; k += OP_WG)
      if (!s_done[k] && op_before(s_reach[k], s_row[k], r, row)) { r = s_reach[k]; row = s_row[k]; pos = k; }
    op_wg_argmin(r, row, pos, sh);
    if (pos < 0) break;                                             // (cannot happen: step < m rows are unprocessed)
    if (tid == 0) {
      s_done[pos] = 1;
      a.ordering[base + step] = row;
    }
    if (a.is_core[row]) {
      const float cdp = a.cd[row];
      for (int k = wave; k < m; k += OP_WG / 64) {
        if (k == pos || s_done[k]) continue;
        const float rn = op_reach_from(a, row, cdp, s_row[k], lane);
        if (lane == 0 && rn >= 0.f && rn < s_reach[k]) { s_reach[k] = rn; s_pred[k] = row; }
      }
    }
    __syncthreads();
  }
  for (int k = tid; k < m; k += OP_WG) {
    a.reach[s_row[k]] = s_reach[k];
    a.pred[s_row[k]] = s_pred[k];
  }
}

// host loop, one step: workgroup b picks for cluster large[b]
__global__ __launch_bounds__(OP_WG) void op_pick_large(OpArgs a, int step) {
  __shared__ int sh[3 * (OP_WG / 64)];
  const int c = a.large[blockIdx.x];
  const int m = a.csize[c];
  if (step >= m) return;
  const int base = a.segoff[c];
  float r = INFINITY;
  int row = INT_MAX, pos = -1;
  for (int k = threadIdx.x; k < m; k += OP_WG) {
    const int j = a.seg_row[base + k];
    if (!a.done[j]) {
      const float rj = a.reach[j];
      if (op_before(rj, j, r, row)) { r = rj; row = j; pos = k; }
    }
  }
  op_wg_argmin(r, row, pos, sh);
  if (threadIdx.x == 0 && pos >= 0) {
    a.done[row] = 1;
    a.ordering[base + step] = row;
    a.cur[blockIdx.x] = row;
  }
}

// host loop, one step: one wave per row (k = its first, + 4 gridDim.x, ...) of cluster large[b] (b = blockIdx.y, + gridDim.y, ...) against
// the row picked in this step
__global__ __launch_bounds__(256) void op_relax_large(OpArgs a, int step, int n_large) {
  const int lane = threadIdx.x & 63;
  for (int b = blockIdx.y; b < n_large; b += gridDim.y) {
    const int c = a.large[b];
    const int m = a.csize[c];
    if (step >= m) continue;
    const int p = a.cur[b];
    if (!a.is_core[p]) continue;
    const float cdp = a.cd[p];
    const int base = a.segoff[c];
    for (int k = blockIdx.x * 4 + (threadIdx.x >> 6); k < m; k += 4 * gridDim.x) {
      const int j = a.seg_row[base + k];
      if (a.done[j]) continue;                                      // (the picked row included)
      const float rn = op_reach_from(a, p, cdp, j, lane);
      if (lane == 0 && rn >= 0.f && rn < a.reach[j]) { a.reach[j] = rn; a.pred[j] = p; }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------

struct OpLayout {
  DbLayout db;                 // first: the label passes' layout (stats and meta at the workspace's start)
  int* ometa; int32_t* knn; float* knn_dist; void* topk_ws;
  int* csize; int* cstart; int* cursor; int* segoff; int* seg_row; int* done; int* large; int* cur;
  float* cd; uint8_t* core; int32_t* ncl;                           // stand-ins for outputs the caller did not ask for
};

static size_t op_layout(void* base, int64_t N, int Dp, int k, OpLayout* L) {
  OpLayout l;
  const size_t dbb = db_layout(base, N, Dp, &l.db);
  SlicCarver c(base ? (char*)base + dbb : nullptr);
  l.ometa = c.take<int>(8);
  l.ncl = c.take<int32_t>(1);
  l.knn = c.take<int32_t>((size_t)N * k);
  l.knn_dist = c.take<float>((size_t)N * k);
  l.topk_ws = c.take<char>(slic_cosine_topk_workspace_bytes((int)N, (int)N, k));
  l.csize = c.take<int>(N);
  l.cstart = c.take<int>(N);
  l.cursor = c.take<int>(N);
  l.segoff = c.take<int>(N);
  l.seg_row = c.take<int>(N);
  l.done = c.take<int>(N);
  l.large = c.take<int>(N);
  l.cur = c.take<int>(N);
  l.cd = c.take<float>(N);
  l.core = c.take<uint8_t>(N);
  if (L) *L = l;
  return dbb + c.off;
}

static int op_k(int min_samples) { return std::min(std::max(min_samples - 1, 1), OP_KMAX); }

extern "C" size_t slic_optics_cosine_workspace_bytes(int64_t N, int D, int min_samples) {
  if (!db_size_ok(N, D) || min_samples < 2 || min_samples > N || min_samples - 1 > OP_KMAX) return 0;
  return op_layout(nullptr, N, (D + 7) / 8 * 8, op_k(min_samples), nullptr);
}

// the last call's host-side record for slic_optics_cosine_stats
static hipEvent_t op_ev[OP_NEV];
static struct { bool timed, cored, walked; int steps, launches, n_large, largest, n_clusters; } op_last;

extern "C" int slic_optics_cosine(const float* X, int64_t N, int ldx, int D, double max_eps, int min_samples, int32_t* labels,
                                  uint8_t* is_core, float* core_dist, float* reachability, int32_t* predecessor, int32_t* ordering,
                                  int32_t* n_clusters, void* workspace, void* stream) {
  SLIC_REQUIRE(D >= 1 && D <= 512, "slic_optics_cosine: D = %d (1 <= D <= 512)", D);
  SLIC_REQUIRE(max_eps >= 0.0 && std::isfinite(max_eps), "slic_optics_cosine: max_eps = %g (finite, >= 0)", max_eps);
  SLIC_REQUIRE(N >= 1 && db_size_ok(N, D), "slic_optics_cosine: N = %lld rows of D = %d (1 <= N, int32 row indices, N x Dp x 4 bytes < 4 GiB)",
               (long long)N, D);
  SLIC_REQUIRE(min_samples >= 2 && min_samples <= N, "slic_optics_cosine: min_samples = %d (2 <= min_samples <= N = %lld)", min_samples,
               (long long)N);
  SLIC_REQUIRE(min_samples - 1 <= OP_KMAX, "slic_optics_cosine: min_samples = %d (the core-distance search keeps lists of at most %d rows)",
               min_samples, OP_KMAX);
  SLIC_REQUIRE(ldx >= D, "slic_optics_cosine: ldx = %d < D = %d", ldx, D);
  SLIC_REQUIRE(X && labels && workspace, "slic_optics_cosine: NULL argument");
  const bool walk = reachability || predecessor || ordering;
  SLIC_REQUIRE(!walk || (reachability && predecessor && ordering && core_dist),
               "slic_optics_cosine: reachability, predecessor and ordering are given together (with core_dist) or all NULL");
  hipStream_t st = S_(stream);
  const int n = (int)N;
  const int Dp = (D + 7) / 8 * 8;
  const int k = op_k(min_samples);
  OpLayout L;
  op_layout(workspace, N, Dp, k, &L);
  if (!is_core) is_core = L.core;
  if (!n_clusters) n_clusters = L.ncl;
  const char* tenv = getenv("SLIC_OPTICS_TIMING");
  op_last.timed = tenv && tenv[0] == '1';
  op_last.cored = op_last.walked = false;
  op_last.steps = op_last.launches = op_last.n_large = op_last.largest = op_last.n_clusters = 0;
  hipEvent_t* ev = op_last.timed ? op_ev : nullptr;
  if (ev)
    for (int i = 0; i < OP_NEV; ++i)
      if (!op_ev[i]) SLIC_HIP_CHECK(hipEventCreate(&op_ev[i]));

  { int r = db_label_passes(X, n, ldx, D, max_eps, min_samples, labels, is_core, nullptr, n_clusters, L.db, true, ev, st); if (r) return r; }
  if (!core_dist) return SLIC_OK;

  { int r = slic_cosine_topk(L.db.Xn, n, L.db.Xn, n, Dp, k, 1, L.knn, L.knn_dist, L.topk_ws, stream); if (r) return r; }
  op_core_dist<<<(n + 3) / 4, 256, 0, st>>>(L.db.Xn, n, Dp, is_core, L.knn, k, core_dist);
  SLIC_LAUNCH_CHECK();
  if (ev) SLIC_HIP_CHECK(hipEventRecord(ev[DB_NEV], st));
  op_last.cored = true;
  if (!walk) return SLIC_OK;

  int lds_rows = OP_LDS_DEFAULT;
  if (const char* e = getenv("SLIC_OPTICS_LDS_ROWS")) lds_rows = std::min(std::max(atoi(e), 0), OP_LDS_ROWS);
  // the screening band of the walk: |d32 - d64| <= (Dp + 8) u (see op_d32), doubled for margin as the label passes' band is
  const double delta = 2.0 * (Dp + 8) * ldexp(1.0, -24);
  OpArgs a;
  a.Xn = L.db.Xn; a.Dp = Dp; a.X = X; a.ldx = ldx; a.D = D; a.inv = L.db.inv; a.eps = max_eps;
  a.dlo = max_eps >= 2.0 ? (double)INFINITY : max_eps - delta;      // every distance is <= 2
  a.dhi = max_eps >= 2.0 ? (double)INFINITY : max_eps + delta;
  a.is_core = is_core; a.cd = core_dist; a.csize = L.csize; a.segoff = L.segoff; a.seg_row = L.seg_row;
  a.reach = reachability; a.pred = predecessor; a.ordering = ordering; a.done = L.done; a.large = L.large; a.cur = L.cur;
  a.stats = L.db.stats; a.lds_rows = lds_rows;

  const int gn = (int)std::min<int64_t>(4096, slic_cdiv(n, 256));
  op_init<<<gn, 256, 0, st>>>(n, reachability, predecessor, L.csize, L.cstart, L.cursor, L.done, L.ometa);
  SLIC_LAUNCH_CHECK();
  op_sizes<<<gn, 256, 0, st>>>(labels, n, L.csize, L.cstart);
  SLIC_LAUNCH_CHECK();
  op_offsets<<<1, DB_SCAN_T, 0, st>>>(labels, n, L.csize, L.cstart, n_clusters, lds_rows, L.segoff, ordering, L.large, L.ometa);
  SLIC_LAUNCH_CHECK();
  op_place<<<gn, 256, 0, st>>>(labels, n, L.segoff, L.cursor, L.seg_row);
  SLIC_LAUNCH_CHECK();
  int meta[4];
  SLIC_HIP_CHECK(hipMemcpyAsync(meta, L.ometa, sizeof(meta), hipMemcpyDeviceToHost, st));
  SLIC_HIP_CHECK(hipStreamSynchronize(st));
  const int ncl = meta[0], nlarge = meta[1], maxlarge = meta[2];
  SLIC_REQUIRE(ncl >= 0 && ncl <= n && nlarge >= 0 && nlarge <= ncl && maxlarge >= 0 && maxlarge <= n,
               "slic_optics_cosine: cluster summary out of range (%d clusters, %d large, largest %d of %d rows)", ncl, nlarge, maxlarge, n);
  int launches = 0;
  if (ncl > nlarge) {
    if (nlarge > 0) a.lds_rows = std::min(lds_rows, OP_LDS_SMALL);      // op_offsets' rule
    op_walk_small<<<ncl, OP_WG, 0, st>>>(a);
    SLIC_LAUNCH_CHECK();
    ++launches;
  }
  if (nlarge > 0) {
    const int gy = std::min(nlarge, 65535);
    const dim3 rg(std::min((maxlarge + 3) / 4, std::max(1, OP_RELAX_WGS / gy)), gy);
    for (int step = 0; step < maxlarge; ++step) {
      op_pick_large<<<nlarge, OP_WG, 0, st>>>(a, step);
      op_relax_large<<<rg, 256, 0, st>>>(a, step, nlarge);
      launches += 2;
    }
    SLIC_LAUNCH_CHECK();
  }
  if (ev) SLIC_HIP_CHECK(hipEventRecord(ev[DB_NEV + 1], st));
  op_last.walked = true;
  op_last.steps = meta[3];
  op_last.launches = launches;
  op_last.n_large = nlarge;
  op_last.largest = meta[3];
  op_last.n_clusters = ncl;
  return SLIC_OK;
}

extern "C" int slic_optics_cosine_stats(const void* workspace, double* out_host, void* stream) {
  SLIC_REQUIRE(workspace && out_host, "slic_optics_cosine_stats: NULL argument");
  hipStream_t st = S_(stream);
  unsigned long long s[DB_NSTAT];
  int meta[8];
  DbLayout L;
  db_layout(const_cast<void*>(workspace), 1, 8, &L);          // stats and meta sit at fixed offsets whatever N and D
  SLIC_HIP_CHECK(hipMemcpyAsync(s, L.stats, sizeof(s), hipMemcpyDeviceToHost, st));
  SLIC_HIP_CHECK(hipMemcpyAsync(meta, L.meta, sizeof(meta), hipMemcpyDeviceToHost, st));
  SLIC_HIP_CHECK(hipStreamSynchronize(st));
  out_host[0] = (double)s[0];
  out_host[1] = (double)s[2];
  out_host[2] = meta[1];
  out_host[3] = op_last.walked ? op_last.n_clusters : -1;
  out_host[4] = op_last.walked ? op_last.largest : -1;
  out_host[5] = op_last.walked ? op_last.steps : 0;
  out_host[6] = op_last.walked ? op_last.launches : 0;
  out_host[7] = op_last.walked ? op_last.n_large : 0;
  for (int i = 0; i < OP_NEV - 1; ++i) {
    float ms = -1.f;
    const bool have = op_last.timed && (i < DB_NEV - 1 || (i == DB_NEV - 1 ? op_last.cored : op_last.walked));
    if (have) SLIC_HIP_CHECK(hipEventElapsedTime(&ms, op_ev[i], op_ev[i + 1]));
    out_host[8 + i] = ms;
  }
  return SLIC_OK;
}
