// Cluster-quality metrics of the cluster step: sklearn.metrics.normalized_mutual_info_score and adjusted_mutual_info_score
// (average_method='arithmetic') of two int32 labellings, finished on the device.
//
// Stands in for the host tail of the reference's online_train.py:605-662 (rank 0 alone in sklearn's expected_mutual_information, a
// triple loop over classes x clusters x n_ij on one host thread).  The contract, the rules and the summation order are in
// include/slic_hip.h (slic_cluster_metrics).
//
// Passes (one stream, no host synchronisation: every size that depends on the data is read from `meta` on the device):
//   ids      per labelling: keys = label with the sign bit flipped (unsigned order = signed order); LSD radix sort, 8 passes of 4 bits,
//            each thread owning CM_CHUNK consecutive keys (16 byte-wide counters packed in two 64-bit registers, so a pass is
//            histogram -> one-workgroup scan (slic_wg_scan_array, wg_scan.h) -> stable scatter with no atomics); run heads of the
//            sorted keys -> scan -> the sorted distinct values uniq[U] and their first positions start[U]; counts = differences of
//            start (the marginal, exact); id[i] = lower bound of key[i] in uniq.
//   table    status = R * C > max_cells; clear R * C cells; n[id_true[i]][id_pred[i]] += 1 (int32 atomics: exact in any order).
//   lgamma   L[x] = lgamma(x + 1), ln[x] = log(x) (ln[0] = 0) and T[x] = sum_{k < x} log1p(-k / N) (a fixed-order scan) for x = 0 .. N.
//   MI, H    one term per cell / class, summed in the fixed order of the header.
//   EMI      one thread per (class, cluster) cell walks n = max(1, a + b - N) .. min(a, b): five table look-ups, one division and one
//            exp per term; cells are dealt round-robin to 1024 x 256 threads.  The work is sum_ij min(a_i, b_j) terms.
//   finish   folds (slic_wg_fold) the four sets of 1024 partial sums and applies the NMI / AMI rules; writes the record.
// fp contraction is off for the whole file: a * b + c stays two roundings, which is what the fp64 check restates on the host.
#include "label_ids.h"
#include "wg_scan.h"
#include <math.h>
#include <float.h>

#pragma clang fp contract(off)

#define CM_CHUNK SLIC_LABEL_CHUNK   // keys per thread in a radix pass
#define CM_G 1024             // workgroups of a fixed-order sum
#define CM_T 256              // threads per workgroup everywhere but the scan
#define CM_SCAN_T 1024        // threads of the one-workgroup scan

enum { CM_R = 0, CM_C = 1, CM_STATUS = 2, CM_NMETA = 16 };
enum { CM_P_MI = 0, CM_P_HT = 1, CM_P_HP = 2, CM_P_EMI = 3 };

// ord (optional): the row numbers the sort carries along
__global__ __launch_bounds__(CM_T) void cm_keys(const int32_t* __restrict__ labels, int N, uint32_t* __restrict__ keys, int* __restrict__ ord) {
  const int i = blockIdx.x * CM_T + threadIdx.x;
  if (i < N) {
    keys[i] = (uint32_t)labels[i] ^ 0x80000000u;
    if (ord) ord[i] = i;
  }
}

// hist[d * T + t] = how many keys of thread t's chunk carry digit d
__global__ __launch_bounds__(CM_T) void cm_radix_hist(const uint32_t* __restrict__ src, int N, int shift, int* __restrict__ hist, int T) {
  const int t = blockIdx.x * CM_T + threadIdx.x;
  if (t >= T) return;
  const int lo = t * CM_CHUNK, hi = min(N, lo + CM_CHUNK);
  unsigned long long c0 = 0, c1 = 0;
  for (int k = lo; k < hi; ++k) {
    const int d = (int)((src[k] >> shift) & 15u);
    if (d < 8) c0 += 1ull << (8 * d); else c1 += 1ull << (8 * (d - 8));
  }
#pragma unroll
  for (int d = 0; d < 16; ++d) hist[d * T + t] = (int)(((d < 8 ? c0 : c1) >> (8 * (d & 7))) & 255ull);
}

// after the exclusive scan of hist in (digit, thread) order, hist[d * T + t] is where thread t's first key with digit d goes.
// ORD: a payload (the row number) moves with its key; the passes are stable, so equal keys keep their rows ascending.
template <bool ORD>
__global__ __launch_bounds__(CM_T) void cm_radix_scatter(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int N, int shift,
                                                        const int* __restrict__ hist, int T, const int* __restrict__ osrc,
                                                        int* __restrict__ odst) {
  const int t = blockIdx.x * CM_T + threadIdx.x;
  if (t >= T) return;
  const int lo = t * CM_CHUNK, hi = min(N, lo + CM_CHUNK);
  unsigned long long c0 = 0, c1 = 0;
  for (int k = lo; k < hi; ++k) {
    const uint32_t key = src[k];
    const int d = (int)((key >> shift) & 15u);
    const int seen = (int)(((d < 8 ? c0 : c1) >> (8 * (d & 7))) & 255ull);
    const int at = hist[d * T + t] + seen;
    if (at >= 0 && at < N) {
      dst[at] = key;
      if constexpr (ORD) odst[at] = osrc[k];
    }
    if (d < 8) c0 += 1ull << (8 * d); else c1 += 1ull << (8 * (d - 8));
  }
}

// exclusive scan of data[0 .. n) in place by one workgroup; *total = the sum
__global__ __launch_bounds__(CM_SCAN_T) void cm_scan(int* __restrict__ data, int n, int* __restrict__ total) {
  slic_wg_scan_array<CM_SCAN_T, int>(data, n, total);
}

__global__ __launch_bounds__(CM_T) void cm_heads(const uint32_t* __restrict__ sorted, int N, int* __restrict__ flag) {
  const int i = blockIdx.x * CM_T + threadIdx.x;
  if (i < N) flag[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

// pos = the exclusive scan of the head flags: a head at i is distinct value number pos[i]
__global__ __launch_bounds__(CM_T) void cm_uniq(const uint32_t* __restrict__ sorted, const int* __restrict__ pos, int N,
                                               uint32_t* __restrict__ uniq, int* __restrict__ start) {
  const int i = blockIdx.x * CM_T + threadIdx.x;
  if (i >= N) return;
  if (i == 0 || sorted[i] != sorted[i - 1]) {
    const int u = pos[i];
    if (u >= 0 && u < N) { uniq[u] = sorted[i]; start[u] = i; }
  }
}

__global__ __launch_bounds__(CM_T) void cm_counts(const int* __restrict__ start, const int* __restrict__ n_uniq, int N, int* __restrict__ cnt) {
  const int u = blockIdx.x * CM_T + threadIdx.x;
  const int U = min(*n_uniq, N);
  if (u < U) cnt[u] = (u + 1 < U ? start[u + 1] : N) - start[u];
}

__global__ __launch_bounds__(CM_T) void cm_ids(const int32_t* __restrict__ labels, int N, const uint32_t* __restrict__ uniq,
                                              const int* __restrict__ n_uniq, int* __restrict__ ids) {
  const int i = blockIdx.x * CM_T + threadIdx.x;
  if (i >= N) return;
  const uint32_t key = (uint32_t)labels[i] ^ 0x80000000u;
  int lo = 0, hi = min(*n_uniq, N);           // lower bound: the first u with uniq[u] >= key (the key is in the list)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (uniq[mid] < key) lo = mid + 1; else hi = mid;
  }
  ids[i] = lo;
}

__global__ void cm_check(int* __restrict__ meta, int64_t max_cells) {
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[CM_STATUS] = (int64_t)meta[CM_R] * (int64_t)meta[CM_C] > max_cells ? 1 : 0;
}

__global__ __launch_bounds__(CM_T) void cm_clear(int* __restrict__ table, const int* __restrict__ meta) {
  if (meta[CM_STATUS]) return;
  const int64_t cells = (int64_t)meta[CM_R] * meta[CM_C];
  for (int64_t p = (int64_t)blockIdx.x * CM_T + threadIdx.x; p < cells; p += (int64_t)CM_G * CM_T) table[p] = 0;
}

__global__ __launch_bounds__(CM_T) void cm_contingency(const int* __restrict__ idt, const int* __restrict__ idp, int N, int* __restrict__ table,
                                                      const int* __restrict__ meta) {
  if (meta[CM_STATUS]) return;
  const int R = meta[CM_R], C = meta[CM_C];
  const int i = blockIdx.x * CM_T + threadIdx.x;
  if (i >= N) return;
  const int r = idt[i], c = idp[i];
  if (r >= 0 && r < R && c >= 0 && c < C) atomicAdd(table + (int64_t)r * C + c, 1);
}

__global__ __launch_bounds__(CM_T) void cm_tables(int N, double* __restrict__ lg, double* __restrict__ ln, double* __restrict__ tl) {
  const int x = blockIdx.x * CM_T + threadIdx.x;
  if (x > N) return;
  lg[x] = lgamma((double)x + 1.0);
  ln[x] = x > 0 ? log((double)x) : 0.0;
  tl[x] = x < N ? log1p(-((double)x / (double)N)) : 0.0;       // cm_scan_f64 turns this into T(x) = sum_{k < x} log(1 - k / N)
}

// the same in float64: the fixed order of slic_wg_scan_array is part of the contract (T(x) of the header)
__global__ __launch_bounds__(CM_SCAN_T) void cm_scan_f64(double* __restrict__ data, int n) {
  slic_wg_scan_array<CM_SCAN_T, double>(data, n, nullptr);
}

__global__ __launch_bounds__(CM_T) void cm_mi(const int* __restrict__ table, const int* __restrict__ a, const int* __restrict__ b,
                                             const double* __restrict__ ln, const int* __restrict__ meta, int N, double* __restrict__ part) {
  __shared__ double s[CM_T];
  const int R = meta[CM_R], C = meta[CM_C];
  double acc = 0.0;
  if (!meta[CM_STATUS] && R > 1 && C > 1) {
    const int64_t cells = (int64_t)R * C;
    const double dN = (double)N, lnN = ln[N];
    for (int64_t p = (int64_t)blockIdx.x * CM_T + threadIdx.x; p < cells; p += (int64_t)CM_G * CM_T) {
      const int n = table[p];
      if (n <= 0 || n > N) continue;                            // n > N cannot happen; keeps ln[n] inside the table
      const int i = (int)(p / C), j = (int)(p - (int64_t)i * C);
      const double cn = (double)n / dN;
      const double log_outer = (-log((double)((int64_t)a[i] * (int64_t)b[j])) + lnN) + lnN;
      double t = cn * (ln[n] - lnN) + cn * log_outer;
      if (fabs(t) < DBL_EPSILON) t = 0.0;
      acc += t;
    }
  }
  const double r = slic_wg_fold<CM_T>(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// part = the partial sums of sum_u (x_u / N) * (log x_u - log N); the entropy is minus their sum
__global__ __launch_bounds__(CM_T) void cm_entropy(const int* __restrict__ cnt, const int* __restrict__ meta, int which, const double* __restrict__ ln,
                                                  int N, double* __restrict__ part) {
  __shared__ double s[CM_T];
  const int U = min(meta[which], N);
  double acc = 0.0;
  if (!meta[CM_STATUS] && U > 1) {
    const double dN = (double)N, lnN = ln[N];
    for (int u = blockIdx.x * CM_T + threadIdx.x; u < U; u += CM_G * CM_T) {
      const int x = cnt[u];
      if (x < 1 || x > N) continue;                             // cannot happen for a class size; keeps ln[x] inside the table
      acc += ((double)x / dN) * (ln[x] - lnN);
    }
  }
  const double r = slic_wg_fold<CM_T>(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(CM_T) void cm_emi(const int* __restrict__ a, const int* __restrict__ b, const double* __restrict__ lg,
                                              const double* __restrict__ ln, const double* __restrict__ tl, const int* __restrict__ meta, int N,
                                              double* __restrict__ part) {
  __shared__ double s[CM_T];
  const int R = meta[CM_R], C = meta[CM_C];
  double acc = 0.0;
  if (!meta[CM_STATUS] && R > 1 && C > 1) {
    const int64_t cells = (int64_t)R * C;
    const double dN = (double)N, lnN = ln[N];
    for (int64_t p = (int64_t)blockIdx.x * CM_T + threadIdx.x; p < cells; p += (int64_t)CM_G * CM_T) {
      const int i = (int)(p / C), j = (int)(p - (int64_t)i * C);
      const int ai = a[i], bj = b[j];
      if (ai < 1 || bj < 1 || ai > N || bj > N) continue;       // cannot happen for marginals; keeps every index inside the tables
      const int lo = max(1, ai + bj - N), hi = min(ai, bj);
      const double pre = lg[ai] + lg[bj];
      const double la = ln[ai], lb = ln[bj], ta = tl[ai], tb = tl[bj];
      double cell = 0.0;
      for (int n = lo; n <= hi; ++n) {
        const double term1 = (double)n / dN;
        const double term2 = ((lnN + ln[n]) - la) - lb;
        const double g = ((((pre - lg[n]) - lg[ai - n]) - lg[bj - n]) - (double)n * lnN) + ((tl[ai + bj - n] - ta) - tb);
        cell += (term1 * term2) * exp(g);
      }
      acc += cell;
    }
  }
  const double r = slic_wg_fold<CM_T>(acc, s);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(CM_T) void cm_finish(const double* __restrict__ part, const int* __restrict__ meta, double* __restrict__ record) {
  __shared__ double s[CM_T];
  const int t = threadIdx.x;
  double sum[4];
  for (int q = 0; q < 4; ++q) {
    const double* p = part + q * CM_G;
    sum[q] = slic_wg_fold<CM_T>(((p[t] + p[t + CM_T]) + p[t + 2 * CM_T]) + p[t + 3 * CM_T], s);
  }
  if (t != 0) return;
  const int R = meta[CM_R], C = meta[CM_C];
  double mi = 0.0, ht = 0.0, hp = 0.0, emi = 0.0, nmi = 0.0, ami = 0.0;
  if (!meta[CM_STATUS]) {
    if (R > 1 && C > 1) {
      mi = fmax(sum[CM_P_MI], 0.0);
      emi = sum[CM_P_EMI];
    }
    if (R > 1) ht = -sum[CM_P_HT];
    if (C > 1) hp = -sum[CM_P_HP];
    const double normalizer = (ht + hp) / 2.0;
    if (R == 1 && C == 1) {
      nmi = 1.0;
      ami = 1.0;
    } else {
      nmi = mi == 0.0 ? 0.0 : mi / normalizer;
      if (R == 1 || C == 1) {
        ami = 0.0;
      } else {
        double den = normalizer - emi;
        den = den < 0.0 ? fmin(den, -DBL_EPSILON) : fmax(den, DBL_EPSILON);
        double num = mi - emi;
        num = num < 0.0 ? fmin(num, -DBL_EPSILON) : fmax(num, DBL_EPSILON);
        ami = num / den;
      }
    }
  }
  record[0] = mi; record[1] = ht; record[2] = hp; record[3] = emi; record[4] = nmi; record[5] = ami;
  record[6] = (double)R; record[7] = (double)C; record[8] = (double)meta[CM_STATUS];
}

struct CmLayout {
  uint32_t *keys_a, *keys_b, *uniq;
  int *hist, *pos, *start, *idt, *idp, *a, *b, *meta, *table;
  double *lg, *ln, *tl, *part;
};

static bool cm_size_ok(int64_t N, int64_t max_cells) {
  return N >= 1 && N <= SLIC_METRICS_MAX_N && max_cells >= 1 && max_cells <= SLIC_METRICS_MAX_CELLS;
}

static size_t cm_layout(void* base, int64_t N, int64_t max_cells, CmLayout* L) {
  SlicCarver c(base);
  const size_t n = (size_t)N, T = (size_t)slic_cdiv(N, CM_CHUNK);
  CmLayout l;
  l.keys_a = c.take<uint32_t>(n);
  l.keys_b = c.take<uint32_t>(n);
  l.uniq = c.take<uint32_t>(n);
  l.hist = c.take<int>(16 * T);
  l.pos = c.take<int>(n);
  l.start = c.take<int>(n);
  l.idt = c.take<int>(n);
  l.idp = c.take<int>(n);
  l.a = c.take<int>(n);
  l.b = c.take<int>(n);
  l.meta = c.take<int>(CM_NMETA);
  l.lg = c.take<double>(n + 1);
  l.ln = c.take<double>(n + 1);
  l.tl = c.take<double>(n + 1);
  l.part = c.take<double>(4 * CM_G);
  l.table = c.take<int>((size_t)max_cells);
  if (L) *L = l;
  return c.off;
}

extern "C" size_t slic_cluster_metrics_workspace_bytes(int64_t N, int64_t max_cells) {
  if (!cm_size_ok(N, max_cells)) return 0;
  return cm_layout(nullptr, N, max_cells, nullptr);
}

// dense ids of one labelling (ascending value), its class sizes, and the class count in *n_uniq (label_ids.h)
int slic_label_dense_ids(const int32_t* labels, int n, const SlicLabelScratch& L, int* ids, int* cnt, int* n_uniq, hipStream_t st) {
  const int T = (int)slic_cdiv(n, CM_CHUNK);
  const dim3 gn((unsigned)slic_cdiv(n, CM_T)), gt((unsigned)slic_cdiv(T, CM_T));
  const bool ord = L.ord_a && L.ord_b;
  cm_keys<<<gn, CM_T, 0, st>>>(labels, n, L.keys_a, ord ? L.ord_a : nullptr);
  SLIC_LAUNCH_CHECK();
  uint32_t *src = L.keys_a, *dst = L.keys_b;
  int *osrc = L.ord_a, *odst = L.ord_b;
  for (int shift = 0; shift < 32; shift += 4) {
    cm_radix_hist<<<gt, CM_T, 0, st>>>(src, n, shift, L.hist, T);
    SLIC_LAUNCH_CHECK();
    cm_scan<<<1, CM_SCAN_T, 0, st>>>(L.hist, 16 * T, nullptr);
    SLIC_LAUNCH_CHECK();
    if (ord) cm_radix_scatter<true><<<gt, CM_T, 0, st>>>(src, dst, n, shift, L.hist, T, osrc, odst);
    else cm_radix_scatter<false><<<gt, CM_T, 0, st>>>(src, dst, n, shift, L.hist, T, nullptr, nullptr);
    SLIC_LAUNCH_CHECK();
    uint32_t* sw = src; src = dst; dst = sw;
    int* osw = osrc; osrc = odst; odst = osw;
  }
  // eight passes: the sorted keys are back in keys_a (= src), the rows in ord_a
  cm_heads<<<gn, CM_T, 0, st>>>(src, n, L.pos);
  SLIC_LAUNCH_CHECK();
  cm_scan<<<1, CM_SCAN_T, 0, st>>>(L.pos, n, n_uniq);
  SLIC_LAUNCH_CHECK();
  cm_uniq<<<gn, CM_T, 0, st>>>(src, L.pos, n, L.uniq, L.start);
  SLIC_LAUNCH_CHECK();
  cm_counts<<<gn, CM_T, 0, st>>>(L.start, n_uniq, n, cnt);
  SLIC_LAUNCH_CHECK();
  cm_ids<<<gn, CM_T, 0, st>>>(labels, n, L.uniq, n_uniq, ids);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

static int cm_dense_ids(const int32_t* labels, int n, const CmLayout& L, int* ids, int* cnt, int* n_uniq, hipStream_t st) {
  const SlicLabelScratch S = {L.keys_a, L.keys_b, L.uniq, L.hist, L.pos, L.start, nullptr, nullptr};
  return slic_label_dense_ids(labels, n, S, ids, cnt, n_uniq, st);
}

extern "C" int slic_cluster_metrics(const int32_t* labels_true, const int32_t* labels_pred, int64_t N, int64_t max_cells, double* record,
                                    void* workspace, void* stream) {
  SLIC_REQUIRE(cm_size_ok(N, max_cells), "slic_cluster_metrics: N = %lld, max_cells = %lld (1 <= N <= %lld, 1 <= max_cells <= %lld)",
               (long long)N, (long long)max_cells, (long long)SLIC_METRICS_MAX_N, (long long)SLIC_METRICS_MAX_CELLS);
  SLIC_REQUIRE(labels_true && labels_pred && record && workspace, "slic_cluster_metrics: NULL argument");
  hipStream_t st = S_(stream);
  const int n = (int)N;
  CmLayout L;
  cm_layout(workspace, N, max_cells, &L);
  int rc = cm_dense_ids(labels_true, n, L, L.idt, L.a, L.meta + CM_R, st);
  if (rc != SLIC_OK) return rc;
  rc = cm_dense_ids(labels_pred, n, L, L.idp, L.b, L.meta + CM_C, st);
  if (rc != SLIC_OK) return rc;
  const dim3 gn((unsigned)slic_cdiv(n, CM_T));
  cm_check<<<1, 64, 0, st>>>(L.meta, max_cells);
  SLIC_LAUNCH_CHECK();
  cm_clear<<<CM_G, CM_T, 0, st>>>(L.table, L.meta);
  SLIC_LAUNCH_CHECK();
  cm_contingency<<<gn, CM_T, 0, st>>>(L.idt, L.idp, n, L.table, L.meta);
  SLIC_LAUNCH_CHECK();
  cm_tables<<<(unsigned)slic_cdiv(N + 1, CM_T), CM_T, 0, st>>>(n, L.lg, L.ln, L.tl);
  SLIC_LAUNCH_CHECK();
  cm_scan_f64<<<1, CM_SCAN_T, 0, st>>>(L.tl, n + 1);
  SLIC_LAUNCH_CHECK();
  cm_mi<<<CM_G, CM_T, 0, st>>>(L.table, L.a, L.b, L.ln, L.meta, n, L.part + CM_P_MI * CM_G);
  SLIC_LAUNCH_CHECK();
  cm_entropy<<<CM_G, CM_T, 0, st>>>(L.a, L.meta, CM_R, L.ln, n, L.part + CM_P_HT * CM_G);
  SLIC_LAUNCH_CHECK();
  cm_entropy<<<CM_G, CM_T, 0, st>>>(L.b, L.meta, CM_C, L.ln, n, L.part + CM_P_HP * CM_G);
  SLIC_LAUNCH_CHECK();
  cm_emi<<<CM_G, CM_T, 0, st>>>(L.a, L.b, L.lg, L.ln, L.tl, L.meta, n, L.part + CM_P_EMI * CM_G);
  SLIC_LAUNCH_CHECK();
  cm_finish<<<1, CM_T, 0, st>>>(L.part, L.meta, record);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
