// What csrc/optics.hip shares with csrc/dbscan.hip: the float64 pair decision, the size of the one-workgroup scans (slic_wg_scan,
// wg_scan.h), the workspace layout of the label passes and the passes themselves (db_label_passes: prep, count, compact, link, number,
// border); and with csrc/hdbscan.hip the unit-row preparation (db_prep).  The other kernels stay in dbscan.hip.
#pragma once
#include "wg_scan.h"
#include <math.h>

#define DB_B 128              // rows per tile (both operands)
#define DB_SCAN_T 1024        // threads of the one-workgroup scans
#define DB_NSTAT 8
#define DB_NEV 7              // events around the six passes

// the exact decision: float64 dot of the raw rows (lower index first, k ascending), times the float64 inverse norms
__device__ inline bool db_exact(const float* __restrict__ X, int ldx, int D, const double* __restrict__ inv, int i, int j, double eps) {
  const int a = min(i, j), b = max(i, j);
  const float* xa = X + (int64_t)a * ldx;
  const float* xb = X + (int64_t)b * ldx;
  double s = 0.0;
  for (int k = 0; k < D; ++k) s = fma((double)xa[k], (double)xb[k], s);
  double d = 1.0 - s * inv[a] * inv[b];
  d = fmin(fmax(d, 0.0), 2.0);
  return d <= eps;
}

// prep of dbscan.hip and hdbscan.hip, one wave per row: inv[i] = 1 / ||x_i|| in float64 (0 for a zero row), Xn[i] = fp32(x_i * inv[i]),
// zero-padded to Dp columns.  The summation order and the rounding are part of both contracts.  A template: the library is built
// without relocatable device code, so every object that launches it compiles its own copy, and one that does not (optics.o) has none.
template <int = 0>
__global__ __launch_bounds__(256) void db_prep(const float* __restrict__ X, int N, int ldx, int D, int Dp, double* __restrict__ inv,
                                               float* __restrict__ Xn) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* x = X + (int64_t)row * ldx;
  double s = 0.0;
  for (int k = lane; k < D; k += 64) s = fma((double)x[k], (double)x[k], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const double iv = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
  if (lane == 0) inv[row] = iv;
  float* xn = Xn + (int64_t)row * Dp;
  for (int k = lane; k < Dp; k += 64) xn[k] = k < D ? (float)((double)x[k] * iv) : 0.f;
}

struct DbLayout {
  unsigned long long* stats; int* meta; double* inv; float* Xn; float* Xcb; int* cnt;
  int* core_idx; int* border_idx; int* parent; int* cid; int* best;
};

static inline size_t db_layout(void* base, int64_t N, int Dp, DbLayout* L) {
  SlicCarver c(base);
  DbLayout l;
  l.stats = c.take<unsigned long long>(DB_NSTAT);             // first: slic_dbscan_cosine_stats reads it at the workspace's start
  l.meta = c.take<int>(8);
  l.inv = c.take<double>(N);
  l.Xn = c.take<float>((size_t)N * Dp);
  l.Xcb = c.take<float>((size_t)N * Dp);
  l.cnt = c.take<int>(N);
  l.core_idx = c.take<int>(N);
  l.border_idx = c.take<int>(N);
  l.parent = c.take<int>(N);
  l.cid = c.take<int>(N);
  l.best = c.take<int>(N);
  if (L) *L = l;
  return c.off;
}

static inline bool db_size_ok(int64_t N, int D) {
  if (N < 1 || D < 1 || D > 512 || N > (1 << 30) - DB_B) return false;
  const int64_t Dp = (D + 7) / 8 * 8;
  return slic_cdiv(N, DB_B) * DB_B * Dp * 4 < (int64_t)0xFFFFFF00u;     // one 32-bit buffer range holds the rows
}

// The six passes of slic_dbscan_cosine on a workspace laid out by db_layout (arguments already checked).  optics_border: a border row keeps
// its cluster only when the cluster's smallest core row is below it (slic_optics_cosine rule 5).  ev: DB_NEV events recorded between the
// passes, or NULL.
__attribute__((visibility("hidden"))) int db_label_passes(const float* X, int n, int ldx, int D, double eps, int min_samples, int32_t* labels,
                                                          uint8_t* is_core, int32_t* counts, int32_t* n_clusters, const DbLayout& L,
                                                          bool optics_border, hipEvent_t* ev, hipStream_t st);
