// DBSCAN with the cosine metric: sklearn.cluster.DBSCAN(eps, min_samples, metric='cosine').fit(X).labels_ on the device.
//
// Stands in for the reference's clustering/cluster_masks.py:55-61 (sklearn brute-force radius search over N x N cosine distances,
// neighbourhood lists kept on the host).  The contract is in include/slic_hip.h; in short, j is a neighbour of i iff the float64
// distance clip(1 - x_i.x_j * inv_i * inv_j, 0, 2) <= eps (inv = 1 / ||x|| in float64, 0 for a zero row), d(i, i) = 0, a row is core iff
// it has >= min_samples neighbours (itself included), clusters are the connected components of the core rows numbered by their smallest
// member, and a non-core row with a core neighbour takes the smallest cluster number among them.
//
// Passes (all on the normalised, zero-padded rows Xn [N, Dp], Dp = D rounded up to 8):
//   prep    inv[i] in float64, Xn[i] = fp32(x_i * inv[i])
//   count   fused similarity GEMM over the 128 x 128 tiles on or above the diagonal (the matrix loop of topk_collect_qreg: query
//           operand in registers, gallery tile through a 4-stage DMA ring, v_mfma_f32_32x32x2_f32).  Epilogue: a score at or above
//           hi is a neighbour, below lo is not, in between is decided in float64 from the raw rows (a per-lane pending list drained
//           between accumulators).  Each hit adds to both rows: the row side in a register, the column side by ballot + one atomic
//           per gallery row and tile.  The N x N matrix is never written.
//   compact core flags, then one workgroup scan (slic_wg_scan) each gives the core list and the border-candidate list (non-core rows
//           with a neighbour other than themselves: count >= 2); their rows are gathered into Xcb = [Xc; Xb].
//   link    the same GEMM over Xc x Xc (upper triangle); a hit unites its two cores in parent[] by CAS, always hooking the larger
//           root under the smaller, so a component's final root is its smallest member.  A tile whose 256 rows already share one
//           root is skipped before its k loop; in the epilogue cached roots are compared before any atomic.
//   number  pointer jumping to the roots, slic_wg_scan over the root flags gives every root its cluster number.
//   border  Xb x Xc (full rectangle): a hit takes atomicMin of the core's root; the smallest root is the smallest cluster number.
// Every decision is an integer fixed by the float64 rule, so labels, core flags and counts are the same on every run.
// csrc/optics.hip runs the same passes (db_label_passes, declared in dbscan_shared.h with the pieces the two files share) with one more
// test in the border labelling.
#include "mfma_ring.h"
#include "dbscan_shared.h"
#include <math.h>
#include <limits.h>
#include <stdlib.h>
#include <algorithm>

#define DB_PC 32              // band pairs pending per lane
#define DB_SLICE 16           // gallery tiles per workgroup
#define DB_SURE 0x40000000     // pending entry of the link pass that is a neighbour already (row indices < 2^30)

enum { DB_COUNT = 0, DB_LINK = 1, DB_BORDER = 2 };

__device__ __forceinline__ int db_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void db_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with path halving: a non-root's parent only ever moves to one of its ancestors, so the store is safe under races
__device__ int db_find(int* parent, int x) {
  int p = db_ld(parent + x);
  while (p != x) {
    const int gp = db_ld(parent + p);
    if (gp != p) db_st(parent + x, gp);
    x = gp;
    p = db_ld(parent + x);
  }
  return x;
}

// union by hooking the larger root under the smaller; returns the (then) root of the merged component
__device__ int db_unite(int* parent, int a, int b) {
  for (;;) {
    a = db_find(parent, a);
    b = db_find(parent, b);
    if (a == b) return a;
    if (a > b) { const int t = a; a = b; b = t; }
    if (atomicCAS(parent + b, b, a) == b) return a;
  }
}

struct DbArgs {
  const float* Xcb;          // [N, Dp]: Xn for the count pass, [Xc; Xb] for the others
  int Dp;
  const int* meta;           // [0] N, [1] core rows, [2] border candidates
  float hi, lo;              // score >= hi: neighbour; < lo: not; between: float64 decision
  const float* X; int ldx, D; const double* inv; double eps;     // the exact path
  int* cnt;                  // count
  const int* core_idx;       // compact core -> row
  const int* border_idx;     // compact border candidate -> row
  int* parent;               // link (border: compressed roots)
  int* best;                 // border
  unsigned long long* stats; // [0] band rechecks, [1] link tiles skipped
};

// one workgroup = one 128-row query tile (A, in registers) x a slice of up to DB_SLICE gallery tiles (B, through the DMA ring)
template <int NK, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void db_tiles(DbArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(NK % 4 == 0, "a gallery tile is a whole number of ring turns");
  static_assert(DB_B * SLIC_RT_BK == SLIC_RT_TILE, "a ring stage is one DB_B-row tile");
  constexpr bool TRI = MODE != DB_BORDER;
  int* pend = (int*)(lds + 4 * SLIC_RT_TILE);                  // [4 waves][DB_PC][64] gallery rows, one column per lane
  int* groot = pend + 4 * DB_PC * 64;                          // [128] cached roots of the gallery tile
  int* tl = groot + DB_B;                                      // [DB_SLICE] gallery tiles this workgroup computes
  int* sm = tl + DB_SLICE;                                     // [2] root min / max of a tile (link skip)
  const int Dp = p.Dp;
  const int nA = MODE == DB_COUNT ? p.meta[0] : MODE == DB_LINK ? p.meta[1] : p.meta[2];
  const int nB = MODE == DB_COUNT ? p.meta[0] : p.meta[1];
  const float* A = MODE == DB_BORDER ? p.Xcb + (int64_t)p.meta[1] * Dp : p.Xcb;
  const float* B = p.Xcb;
  const int I = blockIdx.x;
  if (I * DB_B >= nA) return;                                  // (workgroup-uniform, before any barrier)
  const int nbt = (nB + DB_B - 1) / DB_B;
  int jbeg = blockIdx.y * DB_SLICE;
  const int jend = min(jbeg + DB_SLICE, nbt);
  if (TRI) jbeg = max(jbeg, I);
  if (jbeg >= jend) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;

  // the gallery tiles to compute; the link pass leaves out a tile whose rows already share one root
  int ntl = 0;
  if constexpr (MODE == DB_LINK) {
    const int arow = I * DB_B + tid;
    const int ar = tid < DB_B && arow < nA ? db_find(p.parent, arow) : -1;
    for (int j = jbeg; j < jend; ++j) {
      if (tid == 0) { sm[0] = INT_MAX; sm[1] = -1; }
      __syncthreads();
      const int brow = j * DB_B + tid - DB_B;
      const int rt = tid < DB_B ? ar : (brow < nB ? db_find(p.parent, brow) : -1);
      if (rt >= 0) { atomicMin(&sm[0], rt); atomicMax(&sm[1], rt); }
      __syncthreads();
      const bool skip = sm[0] == sm[1];
      if (!skip && tid == 0) tl[ntl] = j;
      if (skip && tid == 0) atomicAdd(&p.stats[1], 1ull);
      ntl += skip ? 0 : 1;
      __syncthreads();
    }
    if (ntl == 0) return;
  } else {
    for (int j = jbeg; j < jend; ++j) {
      if (tid == 0) tl[ntl] = j;
      ++ntl;
    }
    __syncthreads();
  }

  int* pq = pend + wave * DB_PC * 64;
  int pc = 0;
  const int q = I * DB_B + 32 * wave + r;
  const bool qvalid = q < nA;
  f32x4 qr[NK][4];
  slic_rt_load_frags<NK>(qr, A + (int64_t)(qvalid ? q : nA - 1) * Dp, Dp, h);
  const SlicRtLane ln = slic_rt_lane(tid, Dp);
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)B, 0, (int)((int64_t)nB * Dp * 4), 0x00020000);
  unsigned goff[4];
  slic_rt_offsets<4>(goff, ln, (unsigned)Dp * 4u);
  // ring step (tile, kt) into `stage`; a tile past the list and a k-tile past Dp come from out of range: zeros
  auto issue = [&](int tile, int kt, int stage) {
    const unsigned gb = tile < ntl ? (unsigned)tl[tile] * (unsigned)(DB_B * Dp * 4) : 0u;
    slic_rt_issue(rs_g, lds + stage * SLIC_RT_TILE, wave, goff, gb, kt, ln.kin(kt) && tile < ntl);
  };

  const float hi = p.hi, lo = p.lo;
  const float NANF = __int_as_float(0x7fc00000);               // a masked score: every comparison is false
  int rowcnt = 0;                                              // count: this lane's hits of its query
  int best = INT_MAX;                                          // border: smallest core root met
  int rq = -1;                                                 // link: a member of the query's component (cached)
  auto drain = [&]() {
    if (pc > 0) {
      int nband = 0;
      for (int j = 0; j < pc; ++j) nband += (pq[j * 64 + lane] & DB_SURE) ? 0 : 1;
      if (nband) atomicAdd(&p.stats[0], (unsigned long long)nband);
      const int ia = MODE == DB_COUNT ? q : MODE == DB_LINK ? p.core_idx[q] : p.border_idx[q];
      for (int j = 0; j < pc; ++j) {
        const int e = pq[j * 64 + lane];
        const int gi = e & ~DB_SURE;
        const int ib = MODE == DB_COUNT ? gi : p.core_idx[gi];
        if ((e & DB_SURE) || db_exact(p.X, p.ldx, p.D, p.inv, ia, ib, p.eps)) {
          if constexpr (MODE == DB_COUNT) {
            ++rowcnt;
            atomicAdd(&p.cnt[gi], 1);                          // (never the row itself: that pair is not in the band)
          } else if constexpr (MODE == DB_LINK) {
            rq = db_unite(p.parent, q, gi);
          } else {
            best = min(best, db_ld(p.parent + gi));
          }
        }
      }
    }
    pc = 0;
  };

  f32x16 acc[4];
  f32x4 a[2][4];
  int gfirst = 0;                                              // link / border: first-level parent of this thread's gallery row
  issue(0, 0, 0);
  issue(0, 1, 1);
  issue(0, 2, 2);
  slic_rt_wait<8>();                                           // step 0 has landed
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) a[0][ct] = *(const f32x4*)&lds[slic_rt_off(32 * ct + r, h)];
  for (int tile = 0; tile < ntl; ++tile) {
    const int J = tl[tile];
    const int g0 = J * DB_B;
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
      if constexpr (MODE != DB_COUNT) {
        // the previous tile's epilogue is over (barrier of kt = 0): one level of parent for the cached roots, published at kt = 2 and
        // visible after the barrier of kt = 3.  Any member of a row's component serves: equal cached values imply one component.
        if (kt == 0) {
          if (tid < DB_B) gfirst = g0 + tid < nB ? db_ld(p.parent + g0 + tid) : -1;
          if constexpr (MODE == DB_LINK)
            if (qvalid && rq < 0) rq = db_ld(p.parent + q);
        } else if (kt == 2) {
          if (tid < DB_B) groot[tid] = gfirst;
        }
      }
      slic_rt_ktile_mfma<false, 4>(acc, a, qr[kt], lds, kt & 3, r, h);
    }
    // ---- epilogue: lane (r, h) holds query q against gallery rows g0 + ct * 32 + (v & 3) + 8 (v >> 2) + 4 h
    const bool diag = TRI && J == I;
    const int gl = g0 + 4 * h;
    if (diag || g0 + DB_B > nB || I * DB_B + DB_B > nA) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int gi = gl + ct * 32 + (v & 3) + 8 * (v >> 2);
          // count: the pair (q, gi) once, gi >= q, and the row itself is its own neighbour (d(i, i) = 0, as sklearn's radius
          // search of X against itself: a zero row included); link: gi > q
          const bool below = diag && (MODE == DB_COUNT ? gi < q : gi <= q);
          if (gi >= nB || !qvalid || below) acc[ct][v] = NANF;
          else if (MODE == DB_COUNT && diag && gi == q) acc[ct][v] = INFINITY;
        }
    }
    int colA = 0, colB = 0;                                    // count: hits of gallery rows (lane / 16, lane % 16) and + 4
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      if (__any(pc > DB_PC - 16)) drain();                      // room for the sixteen scores of this accumulator
      float gm = acc[ct][0];
#pragma unroll
      for (int v = 1; v < 16; ++v) gm = fmaxf(gm, acc[ct][v]);
      if (!__any(gm >= lo)) continue;                          // (NaN: false)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const float s = acc[ct][v];
        const int gi = gl + ct * 32 + (v & 3) + 8 * (v >> 2);
        const bool hit = s >= hi;
        if (!hit && s >= lo) {                                 // the band: decided in float64 after the tile
          pq[pc * 64 + lane] = gi;
          ++pc;
        }
        if constexpr (MODE == DB_COUNT) {
          rowcnt += hit ? 1 : 0;
          const unsigned long long m = __ballot(hit && gi != q);
          colA = lane == ct * 16 + v ? __popcll(m & 0xFFFFFFFFull) : colA;
          colB = lane == ct * 16 + v ? __popcll(m >> 32) : colB;
        } else if constexpr (MODE == DB_LINK) {
          if (hit && groot[gi - g0] != rq) {                   // components not known to be one: unite in the drain
            pq[pc * 64 + lane] = gi | DB_SURE;
            ++pc;
          }
        } else {
          if (hit) best = min(best, groot[gi - g0]);
        }
      }
    }
    if constexpr (MODE == DB_COUNT) {
      const int row0 = g0 + (lane >> 4) * 32 + (lane & 3) + 8 * ((lane >> 2) & 3);
      if (colA) atomicAdd(&p.cnt[row0], colA);
      if (colB) atomicAdd(&p.cnt[row0 + 4], colB);
    }
  }
  drain();
  if constexpr (MODE == DB_COUNT) {
    const int tot = rowcnt + __shfl_xor(rowcnt, 32);
    if (h == 0 && qvalid && tot) atomicAdd(&p.cnt[q], tot);
  } else if constexpr (MODE == DB_BORDER) {
    const int b = min(best, __shfl_xor(best, 32));
    if (h == 0 && qvalid && b != INT_MAX) atomicMin(&p.best[q], b);
  }
  slic_rt_wait<0>();                                           // the trailing all-zero DMAs must land before the workgroup leaves
}

// core flags, labels = -1, and the two compactions (core rows, border candidates) in row order
__global__ __launch_bounds__(DB_SCAN_T) void db_compact(const int* __restrict__ cnt, int N, int min_samples,
                                                        uint8_t* __restrict__ is_core, int32_t* __restrict__ labels,
                                                        int* __restrict__ core_idx, int* __restrict__ border_idx, int* __restrict__ meta) {
  __shared__ int sh[DB_SCAN_T / 64];
  int beg, end;
  slic_run_bounds(N, DB_SCAN_T, threadIdx.x, &beg, &end);
  int nc = 0, nb = 0;
  for (int i = beg; i < end; ++i) {
    const int c = cnt[i];
    const bool core = c >= min_samples;
    nc += core ? 1 : 0;
    nb += !core && c >= 2 ? 1 : 0;
  }
  int oc[1] = {nc}, ob[1] = {nb}, tc[1], tb[1];                  // one value at a time: a pair would double sh
  slic_wg_scan<DB_SCAN_T, 1>(oc, sh, tc);
  slic_wg_scan<DB_SCAN_T, 1>(ob, sh, tb);
  for (int i = beg; i < end; ++i) {
    const int c = cnt[i];
    const bool core = c >= min_samples;
    is_core[i] = core ? 1 : 0;
    labels[i] = -1;
    if (core) core_idx[oc[0]++] = i;
    else if (c >= 2) border_idx[ob[0]++] = i;
  }
  if (threadIdx.x == 0) { meta[1] = tc[0]; meta[2] = tb[0]; }
}

// Xcb = [Xn[core_idx]; Xn[border_idx]], parent[c] = c, best[b] = INT_MAX
__global__ __launch_bounds__(256) void db_gather(const float* __restrict__ Xn, int N, int Dp, const int* __restrict__ meta,
                                                 const int* __restrict__ core_idx, const int* __restrict__ border_idx,
                                                 float* __restrict__ Xcb, int* __restrict__ parent, int* __restrict__ best) {
  const int nc = meta[1], nb = meta[2];
  const int64_t per = Dp / 4;
  const int64_t total = (int64_t)(nc + nb) * per;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / per);
    const int c4 = (int)(e - (int64_t)row * per);
    const int src = row < nc ? core_idx[row] : border_idx[row - nc];
    ((f32x4*)(Xcb + (int64_t)row * Dp))[c4] = ((const f32x4*)(Xn + (int64_t)src * Dp))[c4];
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    if (i < nc) parent[i] = i;
    if (i < nb) best[i] = INT_MAX;
  }
}

__global__ __launch_bounds__(256) void db_compress(int* __restrict__ parent, const int* __restrict__ meta) {
  const int nc = meta[1];
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) {
    int x = db_ld(parent + c);
    while (true) {
      const int y = db_ld(parent + x);
      if (y == x) break;
      x = y;
    }
    db_st(parent + c, x);
  }
}

// cluster number of every root (roots in index order), *n_clusters
__global__ __launch_bounds__(DB_SCAN_T) void db_number(const int* __restrict__ parent, const int* __restrict__ meta, int* __restrict__ cid,
                                                       int32_t* __restrict__ n_clusters) {
  __shared__ int sh[DB_SCAN_T / 64];
  const int nc = meta[1];
  int beg, end;
  slic_run_bounds(nc, DB_SCAN_T, threadIdx.x, &beg, &end);
  int o[1] = {0}, tot[1];
  for (int c = beg; c < end; ++c) o[0] += parent[c] == c ? 1 : 0;
  slic_wg_scan<DB_SCAN_T, 1>(o, sh, tot);
  for (int c = beg; c < end; ++c)
    if (parent[c] == c) cid[c] = o[0]++;
  if (threadIdx.x == 0) *n_clusters = tot[0];
}

__global__ __launch_bounds__(256) void db_label_core(const int* __restrict__ parent, const int* __restrict__ cid, const int* __restrict__ meta,
                                                     const int* __restrict__ core_idx, int32_t* __restrict__ labels) {
  const int nc = meta[1];
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nc; c += gridDim.x * blockDim.x) labels[core_idx[c]] = cid[parent[c]];
}

// best[b] is the smallest root among the border row's core neighbours; a root is its component's smallest core, so cid[root] is the
// smallest cluster number.  optics (slic_optics_cosine rule 5): the row keeps it only when that smallest core row is below the row itself.
__global__ __launch_bounds__(256) void db_label_border(const int* __restrict__ best, const int* __restrict__ cid, const int* __restrict__ meta,
                                                       const int* __restrict__ core_idx, const int* __restrict__ border_idx, int optics,
                                                       int32_t* __restrict__ labels) {
  const int nb = meta[2];
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += gridDim.x * blockDim.x) {
    const int r = best[b];
    const int row = border_idx[b];
    labels[row] = r == INT_MAX || (optics && core_idx[r] > row) ? -1 : cid[r];
  }
}

// ------------------------------------------------------------------------------------------------------------------------------

extern "C" size_t slic_dbscan_cosine_workspace_bytes(int64_t N, int D) {
  if (!db_size_ok(N, D)) return 0;
  return db_layout(nullptr, N, (D + 7) / 8 * 8, nullptr);
}

// per-pass timing for scripts/bench_dbscan.py (SLIC_DBSCAN_TIMING=1 when the call is made): events between the passes
static hipEvent_t db_ev[DB_NEV];      // (slic_dbscan_cosine_stats: out_host[4 .. 9])
static bool db_ev_on = false;

static int db_mark(hipStream_t st, hipEvent_t* ev, int i) {
  if (!ev) return SLIC_OK;
  SLIC_HIP_CHECK(hipEventRecord(ev[i], st));
  return SLIC_OK;
}

template <int MODE>
static int db_launch_tiles(int NK, dim3 grid, size_t lds, hipStream_t st, const DbArgs& a) {
  const auto kern = NK == 4 ? db_tiles<4, MODE> : NK == 8 ? db_tiles<8, MODE> : NK == 12 ? db_tiles<12, MODE> : db_tiles<16, MODE>;
  SLIC_LDS_LIMIT(kern, lds);
  kern<<<grid, dim3(256), lds, st>>>(a);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_dbscan_cosine(const float* X, int64_t N, int ldx, int D, double eps, int min_samples, int32_t* labels,
                                  uint8_t* is_core, int32_t* counts, int32_t* n_clusters, void* workspace, void* stream) {
  SLIC_REQUIRE(D >= 1 && D <= 512, "slic_dbscan_cosine: D = %d (1 <= D <= 512)", D);
  SLIC_REQUIRE(eps >= 0.0, "slic_dbscan_cosine: eps = %g (eps >= 0)", eps);
  SLIC_REQUIRE(min_samples >= 1, "slic_dbscan_cosine: min_samples = %d (>= 1)", min_samples);
  SLIC_REQUIRE(N >= 1 && db_size_ok(N, D), "slic_dbscan_cosine: N = %lld rows of D = %d (1 <= N, int32 row indices, N x Dp x 4 bytes < 4 GiB)",
               (long long)N, D);
  SLIC_REQUIRE(ldx >= D, "slic_dbscan_cosine: ldx = %d < D = %d", ldx, D);
  SLIC_REQUIRE(X && labels && is_core && n_clusters && workspace, "slic_dbscan_cosine: NULL argument");
  DbLayout L;
  db_layout(workspace, N, (D + 7) / 8 * 8, &L);
  const char* tenv = getenv("SLIC_DBSCAN_TIMING");
  db_ev_on = tenv && tenv[0] == '1';
  if (db_ev_on)
    for (int i = 0; i < DB_NEV; ++i)
      if (!db_ev[i]) SLIC_HIP_CHECK(hipEventCreate(&db_ev[i]));
  return db_label_passes(X, (int)N, ldx, D, eps, min_samples, labels, is_core, counts, n_clusters, L, false, db_ev_on ? db_ev : nullptr,
                         S_(stream));
}

int db_label_passes(const float* X, int n, int ldx, int D, double eps, int min_samples, int32_t* labels, uint8_t* is_core, int32_t* counts,
                    int32_t* n_clusters, const DbLayout& L, bool optics_border, hipEvent_t* ev, hipStream_t st) {
  const int Dp = (D + 7) / 8 * 8;
  const int NK = (Dp + 127) / 128 * 4;
  int* cnt = counts ? counts : L.cnt;

  // screening band: |s_fp32 - s_fp64| <= (Dp + 2) u for unit rows, doubled for margin
  const double delta = 2.0 * (Dp + 4) * ldexp(1.0, -24);
  float hi, lo;
  if (eps >= 2.0) {
    hi = lo = -INFINITY;                                       // every distance is <= 2: all pairs are neighbours
  } else {
    const double thi = 1.0 - eps + delta, tlo = 1.0 - eps - delta;
    hi = (float)thi;
    if ((double)hi < thi) hi = nextafterf(hi, INFINITY);       // s >= hi  =>  s >= thi
    lo = (float)tlo;
    if ((double)lo > tlo) lo = nextafterf(lo, -INFINITY);      // s < lo   =>  s < tlo
  }

  SLIC_HIP_CHECK(hipMemsetAsync(L.stats, 0, DB_NSTAT * sizeof(unsigned long long), st));
  SLIC_HIP_CHECK(hipMemcpyAsync(L.meta, &n, sizeof(int), hipMemcpyHostToDevice, st));
  SLIC_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)n * sizeof(int), st));
  { int r = db_mark(st, ev, 0); if (r) return r; }
  db_prep<0><<<(n + 3) / 4, 256, 0, st>>>(X, n, ldx, D, Dp, L.inv, L.Xn);
  SLIC_LAUNCH_CHECK();
  { int r = db_mark(st, ev, 1); if (r) return r; }

  DbArgs a;
  a.Dp = Dp; a.meta = L.meta; a.hi = hi; a.lo = lo;
  a.X = X; a.ldx = ldx; a.D = D; a.inv = L.inv; a.eps = eps;
  a.cnt = cnt; a.core_idx = L.core_idx; a.border_idx = L.border_idx;
  a.parent = L.parent; a.best = L.best; a.stats = L.stats;
  const int T = (n + DB_B - 1) / DB_B;
  const dim3 grid(T, (T + DB_SLICE - 1) / DB_SLICE);
  constexpr size_t LDS = (4 * DB_B * SLIC_RT_BK) * 4 + 4 * DB_PC * 64 * 4 + (DB_B + DB_SLICE + 4) * 4;

  a.Xcb = L.Xn;
  { int r = db_launch_tiles<DB_COUNT>(NK, grid, LDS, st, a); if (r) return r; }
  { int r = db_mark(st, ev, 2); if (r) return r; }
  db_compact<<<1, DB_SCAN_T, 0, st>>>(cnt, n, min_samples, is_core, labels, L.core_idx, L.border_idx, L.meta);
  SLIC_LAUNCH_CHECK();
  const int gb = (int)std::min<int64_t>(4096, slic_cdiv((int64_t)n * Dp / 4, 256));
  db_gather<<<gb, 256, 0, st>>>(L.Xn, n, Dp, L.meta, L.core_idx, L.border_idx, L.Xcb, L.parent, L.best);
  SLIC_LAUNCH_CHECK();
  { int r = db_mark(st, ev, 3); if (r) return r; }
  a.Xcb = L.Xcb;
  { int r = db_launch_tiles<DB_LINK>(NK, grid, LDS, st, a); if (r) return r; }
  { int r = db_mark(st, ev, 4); if (r) return r; }
  const int gn = (int)std::min<int64_t>(4096, slic_cdiv(n, 256));
  db_compress<<<gn, 256, 0, st>>>(L.parent, L.meta);
  SLIC_LAUNCH_CHECK();
  db_number<<<1, DB_SCAN_T, 0, st>>>(L.parent, L.meta, L.cid, n_clusters);
  SLIC_LAUNCH_CHECK();
  db_label_core<<<gn, 256, 0, st>>>(L.parent, L.cid, L.meta, L.core_idx, labels);
  SLIC_LAUNCH_CHECK();
  { int r = db_mark(st, ev, 5); if (r) return r; }
  // border rows: only the candidates the compaction listed (none at min_samples <= 2: every workgroup leaves at once)
  { int r = db_launch_tiles<DB_BORDER>(NK, grid, LDS, st, a); if (r) return r; }
  db_label_border<<<gn, 256, 0, st>>>(L.best, L.cid, L.meta, L.core_idx, L.border_idx, optics_border ? 1 : 0, labels);
  SLIC_LAUNCH_CHECK();
  { int r = db_mark(st, ev, 6); if (r) return r; }
  return SLIC_OK;
}

extern "C" int slic_dbscan_cosine_stats(const void* workspace, double* out_host, void* stream) {
  SLIC_REQUIRE(workspace && out_host, "slic_dbscan_cosine_stats: NULL argument");
  hipStream_t st = S_(stream);
  unsigned long long s[DB_NSTAT];
  int meta[8];
  DbLayout L;
  db_layout(const_cast<void*>(workspace), 1, 8, &L);          // stats and meta sit at fixed offsets whatever N and D
  SLIC_HIP_CHECK(hipMemcpyAsync(s, L.stats, sizeof(s), hipMemcpyDeviceToHost, st));
  SLIC_HIP_CHECK(hipMemcpyAsync(meta, L.meta, sizeof(meta), hipMemcpyDeviceToHost, st));
  SLIC_HIP_CHECK(hipStreamSynchronize(st));
  out_host[0] = (double)s[0];
  out_host[1] = (double)s[1];
  out_host[2] = meta[1];
  out_host[3] = meta[2];
  for (int i = 0; i < DB_NEV - 1; ++i) {
    float ms = -1.f;
    if (db_ev_on) SLIC_HIP_CHECK(hipEventElapsedTime(&ms, db_ev[i], db_ev[i + 1]));
    out_host[4 + i] = ms;
  }
  return SLIC_OK;
}
