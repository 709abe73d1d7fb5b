// Pair statistics: the histogram of the pairwise cosine distances of a set of rows (or of two sets), split into the pairs whose rows
// share a label and the pairs that do not, with the sums behind mean, spread and uniformity of either group.  The N x N matrix is never
// written.  The contract is in include/slic_hip.h (slic_pair_stats); in short, d = clip(1 - x^_i . x^_j, 0, 2) from the fp32 dot of
// the unit rows db_prep makes, bin = min(bins - 1, (int)(d * bins / 2)), group 1 iff both rows carry the same label.
//
// Passes (one stream, no host synchronisation):
//   prep    db_prep (dbscan_shared.h) for X and, in the two-set form, for Y: inv in float64, unit rows in fp32, zero-padded to Dp
//   tiles   ps_tiles: the walk of db_tiles<NK, DB_COUNT> (dbscan.hip) — one workgroup = one 128-row query tile in registers x a slice
//           of up to PS_SLICE gallery tiles through the 4-stage DMA ring, tiles on or above the diagonal in the self form — with a
//           histogram epilogue: the gallery tile's 128 (label, present) pairs are published to LDS on the k-tile schedule dbscan's
//           cached roots use; each of a lane's 64 scores adds one to an int32 LDS counter (a workgroup meets at most
//           128 x 16 x 128 pairs) and its d, d^2 and exp(-2 t d) to six float64 accumulators of the lane, in the walk's order.  After
//           the last tile the LDS table is added to the global uint64 table (integer atomics) and the six accumulators are folded by
//           slic_wg_fold into the workgroup's slot of the workspace.
//   record  ps_record: one workgroup adds the slots in a fixed order (strided runs, then slic_wg_fold) and the table's two rows.
// No floating-point atomic anywhere: two calls on the same input give the same bits.
//
// One LDS table per workgroup.  Flat rows put nearly every pair into a few bins, so a wave's 64 lanes add to the same few words; a table
// per wave (SLIC_PAIR_STATS_TABLES=4, kept for scripts/bench_pair_stats.py; bins <= PS_WAVE_BINS) measured 2 - 5 % faster at 64 bins and
// 0 - 3 % at 256, on flat and on clustered rows alike, less with the order of measurement reversed (profiles/pair_stats.txt):
// a few per cent, not a multiple, so the one layout that serves every `bins` is the one that runs.
#include "mfma_ring.h"
#include "dbscan_shared.h"
#include <math.h>
#include <limits.h>
#include <stdlib.h>

#define PS_SLICE 16           // gallery tiles per workgroup
#define PS_T 256
#define PS_NSUM 6             // d, d^2, e for the two groups
#define PS_REC_T 1024         // threads of the record kernel
#define PS_WAVE_BINS 1024     // up to here a table per wave fits beside the ring: 4 x 2 x 1024 x 4 bytes = 32 KB

struct PsArgs {
  const float* A; const float* B;          // unit rows [nA, Dp], [nB, Dp] (self form: the same array)
  const int32_t* la; const int32_t* lb;    // labels or NULL
  int nA, nB, Dp;
  int self;                                // pairs i < j of one set
  int labeled;                             // both sides carry labels
  int has_ignore; int32_t ignore_label;
  int bins, copies;                        // LDS tables: 1, or 4 (one per wave: measurement only)
  float half, tt;                          // bins / 2; (float)(2 t)
  unsigned long long* hist;                // [2][bins]
  double* part;                            // [workgroups][PS_NSUM]
};

template <int NK>
__global__ __launch_bounds__(PS_T) __attribute__((amdgpu_waves_per_eu(1, 1))) void ps_tiles(PsArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  static_assert(NK % 4 == 0, "a gallery tile is a whole number of ring turns");
  static_assert(DB_B * SLIC_RT_BK == SLIC_RT_TILE, "a ring stage is one DB_B-row tile");
  const int bins = p.bins;
  int2* glab = (int2*)(lds + 4 * SLIC_RT_TILE);                // [128] (label, present) of the gallery tile
  int* tl = (int*)(glab + DB_B);                               // [PS_SLICE] gallery tiles this workgroup computes
  int* lh = tl + PS_SLICE;                                     // [copies][2][bins] counters
  const int Dp = p.Dp, nA = p.nA, nB = p.nB;
  const bool TRI = p.self != 0;
  const int I = blockIdx.x;
  const int nbt = (nB + DB_B - 1) / DB_B;
  int jbeg = blockIdx.y * PS_SLICE;
  const int jend = min(jbeg + PS_SLICE, nbt);
  if (TRI) jbeg = max(jbeg, I);
  if (jbeg >= jend) return;                                    // (workgroup-uniform, before any barrier; its slot stays zero)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int ntl = jend - jbeg;
  if (tid < ntl) tl[tid] = jbeg + tid;
  for (int i = tid; i < p.copies * 2 * bins; i += PS_T) lh[i] = 0;
  __syncthreads();
  int* hw = lh + (p.copies > 1 ? wave * 2 * bins : 0);

  const int q = I * DB_B + 32 * wave + r;
  const bool qvalid = q < nA;
  const int lq = qvalid && p.la ? p.la[q] : 0;
  const bool qok = qvalid && !(p.has_ignore && p.la && lq == p.ignore_label);
  const bool labeled = p.labeled != 0;
  f32x4 qr[NK][4];
  slic_rt_load_frags<NK>(qr, p.A + (int64_t)(qvalid ? q : nA - 1) * Dp, Dp, h);
  const SlicRtLane ln = slic_rt_lane(tid, Dp);
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, (int)((int64_t)nB * Dp * 4), 0x00020000);
  unsigned goff[4];
  slic_rt_offsets<4>(goff, ln, (unsigned)Dp * 4u);
  // ring step (tile, kt) into `stage`; a tile past the list and a k-tile past Dp come from out of range: zeros
  auto issue = [&](int tile, int kt, int stage) {
    const unsigned gb = tile < ntl ? (unsigned)tl[tile] * (unsigned)(DB_B * Dp * 4) : 0u;
    slic_rt_issue(rs_g, lds + stage * SLIC_RT_TILE, wave, goff, gb, kt, ln.kin(kt) && tile < ntl);
  };

  const float half = p.half, tt = p.tt;
  double sd[2] = {0.0, 0.0}, sq[2] = {0.0, 0.0}, se[2] = {0.0, 0.0};
  f32x16 acc[4];
  f32x4 a[2][4];
  int2 gnext = {0, 0};                                         // this thread's gallery row of the coming epilogue
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
      // the previous tile's epilogue is over (barrier of kt = 0): the gallery rows' labels, published at kt = 2 and visible after the
      // barrier of kt = 3.  A row past nB or with the ignored label is not present: it takes part in nothing.
      if (kt == 0) {
        if (tid < DB_B) {
          const int g = g0 + tid;
          const int lg = g < nB && p.lb ? p.lb[g] : 0;
          gnext.x = lg;
          gnext.y = g < nB && !(p.has_ignore && p.lb && lg == p.ignore_label) ? 1 : 0;
        }
      } else if (kt == 2) {
        if (tid < DB_B) glab[tid] = gnext;
      }
      slic_rt_ktile_mfma<false, 4>(acc, a, qr[kt], lds, kt & 3, r, h);
    }
    // ---- epilogue: lane (r, h) holds query q against gallery rows g0 + ct * 32 + (v & 3) + 8 (v >> 2) + 4 h
    const int qlim = TRI && J == I ? q - g0 : -1;              // diagonal tile: only columns above the query's own (i < j)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int c = ct * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
        const int2 gl = glab[c];
        const bool ok = qok && gl.y && c > qlim;
        const int same = labeled && gl.x == lq ? 1 : 0;
        const float d = fminf(fmaxf(1.0f - acc[ct][v], 0.0f), 2.0f);
        const int bin = min(bins - 1, (int)(d * half));
        const float e = expf(-(tt * d));
        atomicAdd(&hw[same * bins + bin], ok ? 1 : 0);         // (no branch: a masked pair adds 0 to a bin that exists)
        const double dd = ok ? (double)d : 0.0, ee = ok ? (double)e : 0.0;
        const double d2 = dd * dd;
        sd[0] += same ? 0.0 : dd;
        sd[1] += same ? dd : 0.0;
        sq[0] += same ? 0.0 : d2;
        sq[1] += same ? d2 : 0.0;
        se[0] += same ? 0.0 : ee;
        se[1] += same ? ee : 0.0;
      }
  }
  slic_rt_wait<0>();                                           // the trailing all-zero DMAs must land before the ring is reused
  __syncthreads();
  for (int i = tid; i < 2 * bins; i += PS_T) {
    int n = 0;
    for (int c = 0; c < p.copies; ++c) n += lh[c * 2 * bins + i];
    if (n) atomicAdd(&p.hist[i], (unsigned long long)n);
  }
  double* fs = (double*)lds;                                   // PS_T doubles of the finished ring
  double* out = p.part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * PS_NSUM;
  const double v0 = slic_wg_fold<PS_T>(sd[0], fs), v1 = slic_wg_fold<PS_T>(sd[1], fs);
  const double v2 = slic_wg_fold<PS_T>(sq[0], fs), v3 = slic_wg_fold<PS_T>(sq[1], fs);
  const double v4 = slic_wg_fold<PS_T>(se[0], fs), v5 = slic_wg_fold<PS_T>(se[1], fs);
  if (tid == 0) {
    out[0] = v0; out[1] = v1; out[2] = v2; out[3] = v3; out[4] = v4; out[5] = v5;
  }
}

// record = n_diff, n_same, sum d (diff, same), sum d^2 (diff, same), sum e (diff, same), status.  Thread t adds the slots t, t + T, ...
// in ascending order; the workgroup folds by halving.  A count is below 2^53, so its float64 sum is exact in any order.
__global__ __launch_bounds__(PS_REC_T) void ps_record(const unsigned long long* __restrict__ hist, int bins, const double* __restrict__ part,
                                                      int64_t nwg, double* __restrict__ record) {
  __shared__ double sh[PS_REC_T];
  const int t = threadIdx.x;
  for (int g = 0; g < 2; ++g) {
    double n = 0.0;
    for (int b = t; b < bins; b += PS_REC_T) n += (double)hist[g * bins + b];
    n = slic_wg_fold<PS_REC_T>(n, sh);
    if (t == 0) record[g] = n;
  }
  for (int k = 0; k < PS_NSUM; ++k) {
    double s = 0.0;
    for (int64_t w = t; w < nwg; w += PS_REC_T) s += part[w * PS_NSUM + k];
    s = slic_wg_fold<PS_REC_T>(s, sh);
    if (t == 0) record[2 + k] = s;
  }
  if (t == 0) record[2 + PS_NSUM] = 0.0;
}

struct PsLayout {
  double* invx; double* invy; float* Xn; float* Yn; double* part;
  int64_t nwg;
};

static bool ps_bins_ok(int bins) { return bins >= 8 && bins <= SLIC_PAIR_STATS_MAX_BINS && (bins & (bins - 1)) == 0; }

// Ny == 0: the self form
static bool ps_size_ok(int64_t Nx, int64_t Ny, int D, int bins) {
  if (!ps_bins_ok(bins) || Nx < 1 || Nx > SLIC_PAIR_STATS_MAX_N || Ny < 0 || Ny > SLIC_PAIR_STATS_MAX_N) return false;
  return db_size_ok(Nx, D) && (Ny == 0 || db_size_ok(Ny, D));
}

static size_t ps_layout(void* base, int64_t Nx, int64_t Ny, int D, PsLayout* L) {
  SlicCarver c(base);
  const size_t dp = (size_t)((D + 7) / 8 * 8);
  PsLayout l;
  l.invx = c.take<double>((size_t)Nx);
  l.Xn = c.take<float>((size_t)Nx * dp);
  l.invy = c.take<double>((size_t)Ny);
  l.Yn = c.take<float>((size_t)Ny * dp);
  l.nwg = slic_cdiv(Nx, DB_B) * slic_cdiv(slic_cdiv(Ny ? Ny : Nx, DB_B), PS_SLICE);
  l.part = c.take<double>((size_t)l.nwg * PS_NSUM);
  if (L) *L = l;
  return c.off;
}

extern "C" size_t slic_pair_stats_workspace_bytes(int64_t Nx, int64_t Ny, int D, int bins) {
  if (!ps_size_ok(Nx, Ny, D, bins)) return 0;
  return ps_layout(nullptr, Nx, Ny, D, nullptr);
}

static int ps_launch_tiles(int NK, dim3 grid, size_t lds, hipStream_t st, const PsArgs& a) {
  const auto kern = NK == 4 ? ps_tiles<4> : NK == 8 ? ps_tiles<8> : NK == 12 ? ps_tiles<12> : ps_tiles<16>;
  SLIC_LDS_LIMIT(kern, lds);
  kern<<<grid, dim3(PS_T), lds, st>>>(a);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_pair_stats(const float* X, int64_t Nx, int64_t ldx, const int32_t* lx, const float* Y, int64_t Ny, int64_t ldy,
                               const int32_t* ly, int D, int bins, int has_ignore, int32_t ignore_label, double t, uint64_t* hist,
                               double* record, void* workspace, void* stream) {
  if (!Y) Ny = 0;
  SLIC_REQUIRE(ps_bins_ok(bins), "slic_pair_stats: bins = %d (a power of two in 8 .. %d)", bins, SLIC_PAIR_STATS_MAX_BINS);
  SLIC_REQUIRE(t > 0.0 && t <= 1e30, "slic_pair_stats: t = %g (0 < t <= 1e30)", t);
  SLIC_REQUIRE(!Y || Ny >= 1, "slic_pair_stats: Ny = %lld rows of Y (>= 1)", (long long)Ny);
  SLIC_REQUIRE(ps_size_ok(Nx, Ny, D, bins),
               "slic_pair_stats: Nx = %lld, Ny = %lld, D = %d (1 <= N <= %lld per side, 1 <= D <= 512, N x Dp x 4 bytes < 4 GiB)",
               (long long)Nx, (long long)Ny, D, (long long)SLIC_PAIR_STATS_MAX_N);
  SLIC_REQUIRE(ldx >= D && ldx <= INT_MAX && (!Y || (ldy >= D && ldy <= INT_MAX)), "slic_pair_stats: row stride outside D .. 2^31 - 1");
  SLIC_REQUIRE(X && hist && record && workspace, "slic_pair_stats: NULL argument");
  hipStream_t st = S_(stream);
  const int Dp = (D + 7) / 8 * 8;
  const int NK = (Dp + 127) / 128 * 4;
  PsLayout L;
  ps_layout(workspace, Nx, Ny, D, &L);
  SLIC_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)2 * bins * sizeof(uint64_t), st));
  SLIC_HIP_CHECK(hipMemsetAsync(L.part, 0, (size_t)L.nwg * PS_NSUM * sizeof(double), st));
  db_prep<0><<<(unsigned)slic_cdiv(Nx, 4), 256, 0, st>>>(X, (int)Nx, (int)ldx, D, Dp, L.invx, L.Xn);
  SLIC_LAUNCH_CHECK();
  if (Y) {
    db_prep<0><<<(unsigned)slic_cdiv(Ny, 4), 256, 0, st>>>(Y, (int)Ny, (int)ldy, D, Dp, L.invy, L.Yn);
    SLIC_LAUNCH_CHECK();
  }
  PsArgs a;
  a.A = L.Xn; a.B = Y ? L.Yn : L.Xn;
  a.la = lx; a.lb = Y ? ly : lx;
  a.nA = (int)Nx; a.nB = Y ? (int)Ny : (int)Nx; a.Dp = Dp;
  a.self = Y ? 0 : 1;
  a.labeled = a.la && a.lb ? 1 : 0;
  a.has_ignore = has_ignore ? 1 : 0; a.ignore_label = ignore_label;
  a.bins = bins;
  // one table per workgroup; SLIC_PAIR_STATS_TABLES=4 keeps one per wave where it fits (scripts/bench_pair_stats.py measures both)
  const char* env = getenv("SLIC_PAIR_STATS_TABLES");
  a.copies = bins <= PS_WAVE_BINS && env && env[0] == '4' ? 4 : 1;
  a.half = (float)(bins / 2); a.tt = (float)(2.0 * t);
  a.hist = (unsigned long long*)hist; a.part = L.part;
  const dim3 grid((unsigned)slic_cdiv(a.nA, DB_B), (unsigned)slic_cdiv(slic_cdiv(a.nB, DB_B), PS_SLICE));
  const size_t lds = (size_t)4 * SLIC_RT_TILE * 4 + DB_B * sizeof(int2) + PS_SLICE * 4 + (size_t)a.copies * 2 * bins * 4;
  { int r = ps_launch_tiles(NK, grid, lds, st, a); if (r) return r; }
  ps_record<<<1, PS_REC_T, 0, st>>>(a.hist, bins, L.part, L.nwg, record);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
