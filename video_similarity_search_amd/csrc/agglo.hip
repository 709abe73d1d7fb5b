// Average-linkage agglomerative clustering with the cosine metric and a distance threshold (include/slic_hip.h, slic_agglo_*).
//
// On unit rows the average of all pairwise cosine distances between clusters A and B is 1 - (S_A . S_B) / (|A| |B|), S = the plain sum
// of a cluster's rows: a cluster is one Dp-vector and a count, a merge is a vector add, and a cluster's nearest cluster is an
// inner-product search over the means M = S / n — slic_cosine_topk as it stands, which returns clip(1 - q.g, 0, 2) on whatever rows it
// is given.  Average linkage is reducible, so every pair of clusters that are each other's nearest neighbour belongs to the greedy
// dendrogram and all such pairs below the threshold merge in one round; a cached nearest neighbour stays valid until that neighbour
// takes part in a merge, so after the first round only the "stale" clusters are searched again.
//
// A round is a chain of small launches on one stream with nothing between them but stream order — no workgroup reads what another
// workgroup of the same launch wrote:
//   scan (3 launches)  live / stale flags -> act[0..A) (live ids, ascending), pos[id], q[0..Q) (stale live ids)
//   gather             M[A, Dp] = S[act] / n, Mq[Q, Dp] = S[q] / n
//   slic_cosine_topk   the 2 nearest gallery rows of every query (one of them may be the query itself)
//   pick               nn[id] (a cluster id), nd[id] of every query
//   mark               leader[a] = a is the lower id of a reciprocal pair below the threshold; the record: pairs, smallest (nd, id)
//   apply              one wave per pair: S[a] += S[b] (each lane its own columns: a fixed order, no float atomics), n[a] += n[b], b dies
//   restale            stale[c] = c merged, or its nn merged or died; the record: live and stale counts of the next round
// and one copy of the 32-byte record to the host, the round's only synchronisation.
#include <stdlib.h>

#include "wg_scan.h"

#define AG_SCAN_T 256                 // threads of a scan workgroup
#define AG_SCAN_PER 4                 // ids per thread
#define AG_SCAN_BLK (AG_SCAN_T * AG_SCAN_PER)
#define AG_REC 4                      // the device record: merges, live, stale, (bits of nd << 32 | id) of the closest live cluster

typedef unsigned long long u64;

struct AggloState {
  float* S;          // [N, Dp] cluster sums (a dead cluster's row is what it was when it died)
  float* M;          // [N, Dp] gallery of a round (A rows used)
  float* Mq;         // [N, Dp] queries of a round (Q rows used)
  float* nd;         // [N] distance to nn
  float* odist;      // [N, 2] search result
  int32_t* oidx;     // [N, 2]
  int32_t* cnt;      // [N] rows of a cluster
  int32_t* live;     // [N] 0 / 1
  int32_t* stale;    // [N] 0 / 1, set only on live clusters
  int32_t* leader;   // [N] 0 / 1, this round's pair leaders
  int32_t* nn;       // [N] nearest other cluster (id), -1 before the first search
  int32_t* parent;   // [N] the cluster b was merged into; parent[r] == r for a root
  int32_t* parent2;  // [N] second buffer of the pointer jumping
  int32_t* act;      // [N]
  int32_t* pos;      // [N]
  int32_t* q;        // [N]
  int32_t* bsum;     // [2 * nb] per scan block: live, stale
  int32_t* boff;     // [2 * nb] exclusive offsets
  u64* rec;          // [AG_REC]
  int32_t* bad;      // [1] rows of zero norm or with a non-finite value
};

static int64_t agglo_scan_blocks(int64_t N) { return slic_cdiv(N, AG_SCAN_BLK); }

static AggloState agglo_carve(void* ws, int64_t N, int Dp, size_t* bytes) {
  SlicCarver w(ws);
  AggloState s;
  const size_t n = (size_t)N, nb = (size_t)agglo_scan_blocks(N);
  s.S = w.take<float>(n * Dp);
  s.M = w.take<float>(n * Dp);
  s.Mq = w.take<float>(n * Dp);
  s.nd = w.take<float>(n);
  s.odist = w.take<float>(2 * n);
  s.oidx = w.take<int32_t>(2 * n);
  s.cnt = w.take<int32_t>(n);
  s.live = w.take<int32_t>(n);
  s.stale = w.take<int32_t>(n);
  s.leader = w.take<int32_t>(n);
  s.nn = w.take<int32_t>(n);
  s.parent = w.take<int32_t>(n);
  s.parent2 = w.take<int32_t>(n);
  s.act = w.take<int32_t>(n);
  s.pos = w.take<int32_t>(n);
  s.q = w.take<int32_t>(n);
  s.bsum = w.take<int32_t>(2 * nb);
  s.boff = w.take<int32_t>(2 * nb);
  s.rec = w.take<u64>(AG_REC);
  s.bad = w.take<int32_t>(1);
  if (bytes) *bytes = w.off;
  return s;
}

static bool agglo_size_ok(int64_t N, int D) {
  if (N < 1 || N > SLIC_AGGLO_MAX_N || D < 1 || D > 512) return false;
  return N * (int64_t)((D + 7) / 8 * 8) * 4 < (1ll << 32);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// start
// ---------------------------------------------------------------------------------------------------------------------------------
// one WAVE per row: a row whose squared norm (float64) is not a positive finite number is an argument error
__global__ __launch_bounds__(256) void agglo_check_rows(const float* __restrict__ X, int64_t N, int D, int ldx, int32_t* __restrict__ bad) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  const float* x = X + row * ldx;
  double s = 0.0;
  for (int c = lane; c < D; c += 64) { const double v = (double)x[c]; s += v * v; }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0 && !(s > 0.0 && s < INFINITY)) atomicAdd(bad, 1);
}

// S[row] = the normalised row (dense [N, D]) zero-padded to Dp, and every cluster is one live, stale row
__global__ __launch_bounds__(256) void agglo_init_state(const float* __restrict__ Xn, int64_t N, int D, int Dp, AggloState s) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int lane = threadIdx.x & 63;
  if (Xn != s.S)
    for (int c = lane; c < Dp; c += 64) s.S[row * Dp + c] = c < D ? Xn[row * D + c] : 0.f;
  if (lane == 0) {
    s.cnt[row] = 1; s.live[row] = 1; s.stale[row] = 1; s.leader[row] = 0;
    s.nn[row] = -1; s.nd[row] = INFINITY; s.parent[row] = (int32_t)row;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// scan: act / pos / q from the live and stale flags
// ---------------------------------------------------------------------------------------------------------------------------------
// the workgroup scans one (live, stale) pair per thread in one pass: slic_wg_scan<AG_SCAN_T, 2> (wg_scan.h)

__global__ __launch_bounds__(AG_SCAN_T) void agglo_scan_count(int64_t N, AggloState s) {
  const int64_t i0 = (int64_t)blockIdx.x * AG_SCAN_BLK + (int64_t)threadIdx.x * AG_SCAN_PER;
  __shared__ int sh[2 * (AG_SCAN_T / 64)];
  int v[2] = {0, 0}, tot[2];
  for (int u = 0; u < AG_SCAN_PER; ++u)
    if (i0 + u < N) { v[0] += s.live[i0 + u]; v[1] += s.stale[i0 + u]; }
  slic_wg_scan<AG_SCAN_T, 2>(v, sh, tot);
  if (threadIdx.x == 0) { s.bsum[2 * blockIdx.x] = tot[0]; s.bsum[2 * blockIdx.x + 1] = tot[1]; }
}

// ONE workgroup: exclusive scan of the nb block totals, AG_SCAN_T at a time with a carry
__global__ __launch_bounds__(AG_SCAN_T) void agglo_scan_blocks_kernel(int nb, AggloState s) {
  __shared__ int sh[2 * (AG_SCAN_T / 64)];
  int cx = 0, cy = 0;
  for (int b0 = 0; b0 < nb; b0 += AG_SCAN_T) {
    const int b = b0 + threadIdx.x;
    int v[2] = {b < nb ? s.bsum[2 * b] : 0, b < nb ? s.bsum[2 * b + 1] : 0}, tot[2];
    slic_wg_scan<AG_SCAN_T, 2>(v, sh, tot);
    if (b < nb) { s.boff[2 * b] = cx + v[0]; s.boff[2 * b + 1] = cy + v[1]; }
    cx += tot[0]; cy += tot[1];
  }
}

__global__ __launch_bounds__(AG_SCAN_T) void agglo_scan_write(int64_t N, AggloState s) {
  const int64_t i0 = (int64_t)blockIdx.x * AG_SCAN_BLK + (int64_t)threadIdx.x * AG_SCAN_PER;
  __shared__ int sh[2 * (AG_SCAN_T / 64)];
  int lv[AG_SCAN_PER], st[AG_SCAN_PER];
  int v[2] = {0, 0}, tot[2];
  for (int u = 0; u < AG_SCAN_PER; ++u) {
    lv[u] = i0 + u < N ? s.live[i0 + u] : 0;
    st[u] = i0 + u < N ? s.stale[i0 + u] : 0;
    v[0] += lv[u]; v[1] += st[u];
  }
  slic_wg_scan<AG_SCAN_T, 2>(v, sh, tot);
  int x = v[0] + s.boff[2 * blockIdx.x];
  int y = v[1] + s.boff[2 * blockIdx.x + 1];
  for (int u = 0; u < AG_SCAN_PER; ++u) {
    if (i0 + u >= N) break;
    if (lv[u]) { s.act[x] = (int32_t)(i0 + u); s.pos[i0 + u] = x; ++x; }
    if (st[u]) { s.q[y] = (int32_t)(i0 + u); ++y; }
  }
}

static int agglo_scan(const AggloState& s, int64_t N, hipStream_t st) {
  const int nb = (int)agglo_scan_blocks(N);
  agglo_scan_count<<<dim3(nb), dim3(AG_SCAN_T), 0, st>>>(N, s);
  SLIC_LAUNCH_CHECK();
  agglo_scan_blocks_kernel<<<dim3(1), dim3(AG_SCAN_T), 0, st>>>(nb, s);
  SLIC_LAUNCH_CHECK();
  agglo_scan_write<<<dim3(nb), dim3(AG_SCAN_T), 0, st>>>(N, s);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the round
// ---------------------------------------------------------------------------------------------------------------------------------
// one WAVE per output row: rows [0, A) of M from act, rows [0, Q) of Mq from q; 16-byte loads and stores (Dp % 8 == 0)
__global__ __launch_bounds__(256) void agglo_gather(int A, int Q, int Dp, AggloState s) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= A + Q) return;
  const int lane = threadIdx.x & 63;
  const int id = r < A ? s.act[r] : s.q[r - A];
  float* dst = r < A ? s.M + (int64_t)r * Dp : s.Mq + (int64_t)(r - A) * Dp;
  const f32x4* src = (const f32x4*)(s.S + (int64_t)id * Dp);
  const float n = (float)s.cnt[id];
  for (int c = lane; c < Dp / 4; c += 64) ((f32x4*)dst)[c] = src[c] / n;
}

// query i: the first of its k <= 2 list entries that is not its own gallery position
__global__ __launch_bounds__(256) void agglo_pick(int A, int Q, int k, AggloState s) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Q) return;
  const int id = s.q[i], own = s.pos[id];
  int nn = -1;
  float nd = INFINITY;
  for (int e = k - 1; e >= 0; --e) {
    const int p = s.oidx[(int64_t)i * k + e];
    if (p != own && p >= 0 && p < A) { nn = s.act[p]; nd = s.odist[(int64_t)i * k + e]; }
  }
  s.nn[id] = nn;
  s.nd[id] = nd;
}

__global__ __launch_bounds__(256) void agglo_mark(int64_t N, float threshold, AggloState s) {
  __shared__ u64 skey[4];
  __shared__ int scnt[4];
  const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
  u64 key = ~0ull;
  int lead = 0;
  if (a < N && s.live[a]) {
    const float d = s.nd[a];
    const int b = s.nn[a];
    key = ((u64)__float_as_uint(d) << 32) | (u64)a;             // d >= 0: its bits order as it does
    if (b > a && b < N && s.live[b] && s.nn[b] == (int)a && d < threshold) lead = 1;
  }
  if (a < N) s.leader[a] = lead;
  for (int o = 32; o > 0; o >>= 1) {
    const u64 ok = __shfl_xor(key, o);
    key = ok < key ? ok : key;
    lead += __shfl_xor(lead, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { skey[w] = key; scnt[w] = lead; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { key = skey[i] < key ? skey[i] : key; lead += scnt[i]; }
    if (lead) atomicAdd(&s.rec[0], (u64)lead);
    if (key != ~0ull) atomicMin(&s.rec[3], key);
  }
}

// the fallback's mark: the closest live cluster i of the record and its neighbour become the one pair of this step
__global__ void agglo_mark_closest(int64_t N, AggloState s) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const u64 key = s.rec[3];
  const int64_t i = (int64_t)(key & 0xFFFFFFFFull);
  if (key == ~0ull || i >= N || !s.live[i]) return;
  const int j = s.nn[i];
  if (j < 0 || j >= N || j == i || !s.live[j]) return;
  const int a = i < j ? (int)i : j, b = i < j ? j : (int)i;
  s.nn[a] = b;
  s.leader[a] = 1;
  s.rec[0] = 1;
}

// one WAVE per id; a leader adds its partner's sum to its own, lane l columns 4 l .. 4 l + 3, 256 + 4 l ..: no other wave touches either row
__global__ __launch_bounds__(256) void agglo_apply(int64_t N, int Dp, AggloState s) {
  const int64_t a = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= N || !s.leader[a]) return;
  const int lane = threadIdx.x & 63;
  const int b = s.nn[a];
  f32x4* sa = (f32x4*)(s.S + a * Dp);
  const f32x4* sb = (const f32x4*)(s.S + (int64_t)b * Dp);
  for (int c = lane; c < Dp / 4; c += 64) sa[c] = sa[c] + sb[c];
  if (lane == 0) {
    s.cnt[a] += s.cnt[b];
    s.live[b] = 0;
    s.parent[b] = (int32_t)a;
  }
}

__global__ __launch_bounds__(256) void agglo_restale(int64_t N, AggloState s) {
  __shared__ int sl[4], ss[4];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int lv = 0, st = 0;
  if (c < N) {
    lv = s.live[c];
    if (lv) {
      const int n = s.nn[c];
      st = (s.leader[c] || n < 0 || n >= N || !s.live[n] || s.leader[n]) ? 1 : 0;
    }
    s.stale[c] = st;
  }
  for (int o = 32; o > 0; o >>= 1) { lv += __shfl_xor(lv, o); st += __shfl_xor(st, o); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sl[w] = lv; ss[w] = st; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { lv += sl[i]; st += ss[i]; }
    if (lv) atomicAdd(&s.rec[1], (u64)lv);
    if (st) atomicAdd(&s.rec[2], (u64)st);
  }
}

static int agglo_record_clear(const AggloState& s, bool keep_closest, hipStream_t st) {
  SLIC_HIP_CHECK(hipMemsetAsync(s.rec, 0, 3 * sizeof(u64), st));
  if (!keep_closest) SLIC_HIP_CHECK(hipMemsetAsync(s.rec + 3, 0xFF, sizeof(u64), st));
  return SLIC_OK;
}

static int agglo_record_read(const AggloState& s, int64_t* record_host, hipStream_t st) {
  u64 h[AG_REC];
  SLIC_HIP_CHECK(hipMemcpyAsync(h, s.rec, sizeof(h), hipMemcpyDeviceToHost, st));
  SLIC_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < AG_REC; ++i) record_host[i] = (int64_t)h[i];
  record_host[AG_REC] = -1;                                      // search time: slic_agglo_round fills it in when asked to measure
  return SLIC_OK;
}

static int agglo_merge_tail(const AggloState& s, int64_t N, int Dp, int64_t* record_host, hipStream_t st) {
  agglo_apply<<<dim3((unsigned)slic_cdiv(N, 4)), dim3(256), 0, st>>>(N, Dp, s);
  SLIC_LAUNCH_CHECK();
  agglo_restale<<<dim3((unsigned)slic_cdiv(N, 256)), dim3(256), 0, st>>>(N, s);
  SLIC_LAUNCH_CHECK();
  return agglo_record_read(s, record_host, st);
}

extern "C" size_t slic_agglo_workspace_bytes(int64_t N, int D) {
  if (!agglo_size_ok(N, D)) return 0;
  size_t b = 0;
  agglo_carve(nullptr, N, (D + 7) / 8 * 8, &b);
  return b;
}

extern "C" int slic_agglo_start(const float* X, int64_t N, int ldx, int D, void* workspace, int32_t* bad_rows_host, void* stream) {
  SLIC_REQUIRE(X && workspace && bad_rows_host, "slic_agglo_start: null pointer");
  SLIC_REQUIRE(agglo_size_ok(N, D) && ldx >= D, "slic_agglo_start: need 1 <= N <= 2^24, 1 <= D <= 512, ldx >= D, < 4 GiB padded (N=%lld D=%d ldx=%d)",
               (long long)N, D, ldx);
  SLIC_REQUIRE(((uintptr_t)workspace % 256) == 0, "slic_agglo_start: the workspace must be 256-byte aligned");
  hipStream_t st = S_(stream);
  const int Dp = (D + 7) / 8 * 8;
  const AggloState s = agglo_carve(workspace, N, Dp, nullptr);
  SLIC_HIP_CHECK(hipMemsetAsync(s.bad, 0, sizeof(int32_t), st));
  const dim3 rows((unsigned)slic_cdiv(N, 4));
  agglo_check_rows<<<rows, dim3(256), 0, st>>>(X, N, D, ldx, s.bad);
  SLIC_LAUNCH_CHECK();
  float* Xn = Dp == D ? s.S : s.M;                               // dense [N, D]: in place when there is no padding
  const int rc = slic_normalize_rows(X, N, D, ldx, Xn, stream);
  if (rc != SLIC_OK) return rc;
  agglo_init_state<<<rows, dim3(256), 0, st>>>(Xn, N, D, Dp, s);
  SLIC_LAUNCH_CHECK();
  SLIC_HIP_CHECK(hipMemcpyAsync(bad_rows_host, s.bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  SLIC_HIP_CHECK(hipStreamSynchronize(st));
  return SLIC_OK;
}

extern "C" int slic_agglo_round(void* workspace, int64_t N, int D, int A, int Q, float threshold, void* topk_workspace,
                                int64_t* record_host, void* stream) {
  SLIC_REQUIRE(workspace && topk_workspace && record_host, "slic_agglo_round: null pointer");
  SLIC_REQUIRE(agglo_size_ok(N, D) && A >= 2 && A <= N && Q >= 0 && Q <= A, "slic_agglo_round: bad sizes (N=%lld D=%d A=%d Q=%d)",
               (long long)N, D, A, Q);
  hipStream_t st = S_(stream);
  const int Dp = (D + 7) / 8 * 8;
  const AggloState s = agglo_carve(workspace, N, Dp, nullptr);
  int rc = agglo_record_clear(s, false, st);
  if (rc != SLIC_OK) return rc;
  // SLIC_AGGLO_TIMING=1 (measurement only): device events around the search, read after the round's one synchronisation
  const char* te = getenv("SLIC_AGGLO_TIMING");
  const bool timing = te && te[0] == '1' && Q > 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (timing) {
    SLIC_HIP_CHECK(hipEventCreate(&e0));
    SLIC_HIP_CHECK(hipEventCreate(&e1));
  }
  if (Q > 0) {
    if ((rc = agglo_scan(s, N, st)) != SLIC_OK) return rc;
    agglo_gather<<<dim3((unsigned)slic_cdiv((int64_t)A + Q, 4)), dim3(256), 0, st>>>(A, Q, Dp, s);
    SLIC_LAUNCH_CHECK();
    if (timing) SLIC_HIP_CHECK(hipEventRecord(e0, st));
    if ((rc = slic_cosine_topk(s.Mq, Q, s.M, A, Dp, 2, 0, s.oidx, s.odist, topk_workspace, stream)) != SLIC_OK) return rc;
    if (timing) SLIC_HIP_CHECK(hipEventRecord(e1, st));
    agglo_pick<<<dim3((unsigned)slic_cdiv(Q, 256)), dim3(256), 0, st>>>(A, Q, 2, s);
    SLIC_LAUNCH_CHECK();
  }
  agglo_mark<<<dim3((unsigned)slic_cdiv(N, 256)), dim3(256), 0, st>>>(N, threshold, s);
  SLIC_LAUNCH_CHECK();
  rc = agglo_merge_tail(s, N, Dp, record_host, st);
  if (timing) {
    float ms = -1.f;
    if (rc == SLIC_OK && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) record_host[AG_REC] = (int64_t)((double)ms * 1e6);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  return rc;
}

extern "C" int slic_agglo_merge_closest(void* workspace, int64_t N, int D, int64_t* record_host, void* stream) {
  SLIC_REQUIRE(workspace && record_host, "slic_agglo_merge_closest: null pointer");
  SLIC_REQUIRE(agglo_size_ok(N, D), "slic_agglo_merge_closest: bad sizes (N=%lld D=%d)", (long long)N, D);
  hipStream_t st = S_(stream);
  const int Dp = (D + 7) / 8 * 8;
  const AggloState s = agglo_carve(workspace, N, Dp, nullptr);
  const int rc = agglo_record_clear(s, true, st);
  if (rc != SLIC_OK) return rc;
  agglo_mark_closest<<<dim3(1), dim3(64), 0, st>>>(N, s);
  SLIC_LAUNCH_CHECK();
  return agglo_merge_tail(s, N, Dp, record_host, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// labels
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void agglo_jump(int64_t N, const int32_t* __restrict__ src, int32_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) dst[i] = src[src[i]];
}

__global__ __launch_bounds__(256) void agglo_write_labels(int64_t N, const int32_t* __restrict__ root, const int32_t* __restrict__ pos,
                                                          int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) labels[i] = pos[root[i]];
}

extern "C" int slic_agglo_labels(void* workspace, int64_t N, int D, int32_t* labels, void* stream) {
  SLIC_REQUIRE(workspace && labels, "slic_agglo_labels: null pointer");
  SLIC_REQUIRE(agglo_size_ok(N, D), "slic_agglo_labels: bad sizes (N=%lld D=%d)", (long long)N, D);
  hipStream_t st = S_(stream);
  const AggloState s = agglo_carve(workspace, N, (D + 7) / 8 * 8, nullptr);
  // a chain of parents is at most N - 1 long and halves with every jump; the state's own parent array is left as it is
  const dim3 grid((unsigned)slic_cdiv(N, 256));
  SLIC_HIP_CHECK(hipMemcpyAsync(s.parent2, s.parent, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  int32_t* cur = s.parent2;
  int32_t* nxt = s.act;                                          // act is rewritten by the scan below, after the last jump
  for (int64_t len = 1; len < N; len <<= 1) {
    agglo_jump<<<grid, dim3(256), 0, st>>>(N, cur, nxt);
    SLIC_LAUNCH_CHECK();
    int32_t* t = cur; cur = nxt; nxt = t;
  }
  if (cur != s.parent2) SLIC_HIP_CHECK(hipMemcpyAsync(s.parent2, cur, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  const int rc = agglo_scan(s, N, st);                           // pos[root] = the root's rank among the live clusters
  if (rc != SLIC_OK) return rc;
  agglo_write_labels<<<grid, dim3(256), 0, st>>>(N, s.parent2, s.pos, labels);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
