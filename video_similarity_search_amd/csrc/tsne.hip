// Exact t-SNE with a dense N x N matrix P of joint probabilities, and the centred Gram matrix of PCA (contract in
// include/slic_hip.h, slic_tsne_*; DESIGN section 7, "t-SNE and PCA").  fp32 storage, plain HIP C++; every N^2-sized index is int64;
// every loop bound is a kernel argument; no floating-point atomics: every sum has one fixed order, so two runs give the same bits.
//
// Once per fit:
//   sqdist       d2[i][j] = sum_k (x_ik - x_jk)^2, k ascending, on 64 x 64 tiles with 16-column slabs of both row blocks in LDS.
//                The direct form: a duplicate row gives exactly 0, the diagonal is exactly 0.
//   cond_p       one workgroup per row, in place over d2: sklearn's _binary_search_perplexity (dense case: at most 100 steps,
//                |H - log perplexity| <= 1e-5, beta from 1 by doubling / halving / bisection, the diagonal left out) on distances
//                shifted by the row's smallest off-diagonal one: the same P, and sum p >= 1 whatever beta is.  The row sits in LDS
//                (its first TSNE_ROW_LDS floats; the rest is re-read); sum p and sum p (d - dmin) are float64.
//   symmetrize   sum P in float64 (TSNE_G strided partial sums folded by halving, then one fold), then tiles (a, b) and (b, a)
//                together: P <- max((P + P^T) / 2 sum P, DBL_EPSILON), the diagonal 0.
// Per iteration, three launches:
//   forces       workgroup = 16 rows x one share of the columns; lanes run along j (row i of P is read coalesced), a wave carries
//                four rows so that one LDS read of y_j serves four pairs; the share's y in LDS slab by slab.  Per row and share:
//                the attractive and repulsive sums (fp32), Z_i and on request sum P log P, sum P log w, sum P (float64).
//   update       every workgroup folds the N x shares values of Z_i in float64 in one order (the same bits in every workgroup),
//                then for its 256 rows: grad = 4 (attr - rep / Z), sklearn's gains / momentum rule, Y += update; per workgroup
//                the float64 partial sums of |gain grad|^2 and of the KL pieces
//   record       one workgroup: the partial sums folded, the record written
#include "wg_scan.h"
#include <float.h>
#include <math.h>

#define TSNE_T 256
#define TSNE_G 1024              // workgroups of the strided sum of P
#define TSNE_ROW_LDS 40000       // floats of a row of d2 that cond_p keeps in LDS (160 000 of the 163 840 bytes)
#define TSNE_STEPS 100           // sklearn: n_steps
#define TSNE_FR 16               // rows per workgroup of the forces kernel (4 waves x 4 rows)
#define TSNE_FJ 2048             // columns of y per LDS slab
#define TSNE_MAX_SPLIT 16        // column shares
#define TSNE_MAX_BLOCKS 256      // update workgroups at N = 65 536

static bool tsne_size_ok(int64_t N) { return N >= 2 && N <= SLIC_TSNE_MAX_N; }

// ---------------------------------------------------------------- squared distances
__global__ __launch_bounds__(TSNE_T) void tsne_sqdist(const float* __restrict__ X, int N, int D, int64_t ldx, float* __restrict__ d2) {
  __shared__ float A[64][17], B[64][17];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < D; k0 += 16) {
    for (int e = tid; e < 64 * 16; e += TSNE_T) {
      const int r = e >> 4, k = k0 + (e & 15);
      const int i = i0 + r, j = j0 + r;
      A[r][e & 15] = (i < N && k < D) ? X[(int64_t)i * ldx + k] : 0.f;
      B[r][e & 15] = (j < N && k < D) ? X[(int64_t)j * ldx + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float xa[4], xb[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) xa[a] = A[ty + 16 * a][k];
#pragma unroll
      for (int b = 0; b < 4; ++b) xb[b] = B[tx + 16 * b][k];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float d = xa[a] - xb[b];
          acc[a][b] = fmaf(d, d, acc[a][b]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < N && j < N) d2[(int64_t)i * N + j] = acc[a][b];
    }
}

// ---------------------------------------------------------------- conditional probabilities
__global__ __launch_bounds__(TSNE_T) void tsne_cond_p(float* __restrict__ P, int N, double desired_entropy, float* __restrict__ beta_out) {
  extern __shared__ __attribute__((aligned(16))) float tsne_row[];
  __shared__ double sh[TSNE_T];
  const int i = blockIdx.x, t = threadIdx.x;
  float* row = P + (int64_t)i * N;
  const int nl = N < TSNE_ROW_LDS ? N : TSNE_ROW_LDS;
  float mn = INFINITY;
  for (int j = t; j < N; j += TSNE_T) {
    const float d = row[j];
    if (j < nl) tsne_row[j] = d;
    if (j != i) mn = fminf(mn, d);
  }
  sh[t] = (double)mn;
  __syncthreads();
  for (int o = TSNE_T / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] = fmin(sh[t], sh[t + o]);
    __syncthreads();
  }
  const float dmin = (float)sh[0];
  __syncthreads();
  for (int j = t; j < N; j += TSNE_T) {                         // the shifted row replaces the distances
    const float d = (j < nl ? tsne_row[j] : row[j]) - dmin;
    if (j < nl) tsne_row[j] = d; else row[j] = d;
  }
  __syncthreads();
  double beta = 1.0, beta_used = 1.0, beta_min = -INFINITY, beta_max = INFINITY, sum_p = 1.0;
  for (int l = 0; l < TSNE_STEPS; ++l) {
    beta_used = beta;
    const float nb = -(float)beta;
    double sp = 0.0, sdp = 0.0;
    for (int j = t; j < N; j += TSNE_T) {
      if (j == i) continue;
      const float d = j < nl ? tsne_row[j] : row[j];
      const float p = expf(nb * d);
      sp += (double)p;
      sdp += (double)p * (double)d;
    }
    sum_p = slic_wg_fold<TSNE_T>(sp, sh);
    const double sum_dp = slic_wg_fold<TSNE_T>(sdp, sh);
    if (sum_p == 0.0) sum_p = 1e-8;
    const double diff = log(sum_p) + beta * (sum_dp / sum_p) - desired_entropy;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
  // the row of the last step evaluated, as sklearn leaves it (after 100 steps without a break beta itself has moved once more)
  const float nb = -(float)beta_used;
  double sp = 0.0;
  for (int j = t; j < N; j += TSNE_T) {
    if (j == i) continue;
    const float d = j < nl ? tsne_row[j] : row[j];
    sp += (double)expf(nb * d);
  }
  sum_p = slic_wg_fold<TSNE_T>(sp, sh);
  if (sum_p == 0.0) sum_p = 1e-8;
  for (int j = t; j < N; j += TSNE_T) {
    const float d = j < nl ? tsne_row[j] : row[j];
    row[j] = j == i ? 0.f : (float)((double)expf(nb * d) / sum_p);
  }
  if (t == 0) beta_out[i] = (float)beta_used;
}

// ---------------------------------------------------------------- symmetrise
__global__ __launch_bounds__(TSNE_T) void tsne_sum_part(const float* __restrict__ P, int64_t n, double* __restrict__ part) {
  __shared__ double sh[TSNE_T];
  double acc = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * TSNE_T + threadIdx.x; k < n; k += (int64_t)TSNE_G * TSNE_T) acc += (double)P[k];
  const double r = slic_wg_fold<TSNE_T>(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

__global__ __launch_bounds__(TSNE_T) void tsne_sum_fold(const double* __restrict__ part, double* __restrict__ total) {
  __shared__ double sh[TSNE_T];
  const int t = threadIdx.x;
  const double r = slic_wg_fold<TSNE_T>(((part[t] + part[t + TSNE_T]) + part[t + 2 * TSNE_T]) + part[t + 3 * TSNE_T], sh);
  if (t == 0) total[0] = r;
}

// workgroup (bx, by), bx >= by: tiles (by, bx) and (bx, by) of 32 x 32
__global__ __launch_bounds__(TSNE_T) void tsne_sym_apply(float* __restrict__ P, int N, const double* __restrict__ total) {
  __shared__ float U[32][33], L[32][33];
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int r0 = by * 32, c0 = bx * 32;
  for (int r = ty; r < 32; r += 8) {
    const int iu = r0 + r, ju = c0 + tx;                        // upper tile, element (r, tx)
    U[r][tx] = (iu < N && ju < N) ? P[(int64_t)iu * N + ju] : 0.f;
    const int il = c0 + r, jl = r0 + tx;                        // lower tile, element (r, tx)
    L[r][tx] = (il < N && jl < N) ? P[(int64_t)il * N + jl] : 0.f;
  }
  __syncthreads();
  const double inv = 1.0 / fmax(2.0 * total[0], DBL_EPSILON);
  for (int r = ty; r < 32; r += 8) {
    const int iu = r0 + r, ju = c0 + tx;
    if (iu < N && ju < N)
      P[(int64_t)iu * N + ju] = iu == ju ? 0.f : fmaxf((float)(((double)U[r][tx] + (double)L[tx][r]) * inv), (float)DBL_EPSILON);
    const int il = c0 + r, jl = r0 + tx;
    if (bx != by && il < N && jl < N)
      P[(int64_t)il * N + jl] = fmaxf((float)(((double)U[tx][r] + (double)L[r][tx]) * inv), (float)DBL_EPSILON);
  }
}

// ---------------------------------------------------------------- forces
// part[q][share][i]: q = 0 .. 3 the attractive and the repulsive sum (x, y each), fp32; dpart[q][share][i]: q = 0 Z_i, and with KL
// 1 sum P log P, 2 sum P log w, 3 sum P, float64 (a lane's running sum and the wave's butterfly)
template <bool KL>
__global__ __launch_bounds__(TSNE_T) void tsne_forces(const float* __restrict__ P, const float* __restrict__ Y, int N, float exag,
                                                      float* __restrict__ part, double* __restrict__ dpart) {
  __shared__ float2 ys[TSNE_FJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.y, nsplit = gridDim.y;
  // shares are whole multiples of 64 columns, so a lane's columns of one row stay 64 apart
  const int per = ((N + nsplit - 1) / nsplit + 63) / 64 * 64;
  const int c0 = min(split * per, N), c1 = min(c0 + per, N);
  const int ibase = blockIdx.x * TSNE_FR + wave * 4;
  float yix[4], yiy[4];
  const float* prow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = min(ibase + r, N - 1);                        // rows past N repeat the last row and are not written
    yix[r] = Y[2 * (int64_t)i];
    yiy[r] = Y[2 * (int64_t)i + 1];
    prow[r] = P + (int64_t)i * N;
  }
  float ax[4], ay[4], rx[4], ry[4];
  double z[4], plp[4], plw[4], ps[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    ax[r] = ay[r] = rx[r] = ry[r] = 0.f;
    z[r] = plp[r] = plw[r] = ps[r] = 0.0;
  }
  for (int s0 = c0; s0 < c1; s0 += TSNE_FJ) {
    const int sn = min(TSNE_FJ, c1 - s0);
    __syncthreads();
    for (int e = tid; e < sn; e += TSNE_T) ys[e] = make_float2(Y[2 * (int64_t)(s0 + e)], Y[2 * (int64_t)(s0 + e) + 1]);
    __syncthreads();
    for (int e = lane; e < sn; e += 64) {
      const int j = s0 + e;
      const float2 yj = ys[e];
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = prow[r][j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dx = yix[r] - yj.x, dy = yiy[r] - yj.y;
        const float w = 1.0f / (1.0f + fmaf(dx, dx, dy * dy));
        const bool off = j != min(ibase + r, N - 1);            // the pair (i, i) is no pair
        const float pw = exag * p[r] * w, w2 = w * w;
        if (off) z[r] += (double)w;
        ax[r] = fmaf(pw, dx, ax[r]);
        ay[r] = fmaf(pw, dy, ay[r]);
        rx[r] = fmaf(w2, dx, rx[r]);
        ry[r] = fmaf(w2, dy, ry[r]);
        if (KL && off) {
          plp[r] += (double)p[r] * (double)logf(p[r]);
          plw[r] += (double)p[r] * (double)logf(w);
          ps[r] += (double)p[r];
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v[4] = {ax[r], ay[r], rx[r], ry[r]};
    double d[4] = {z[r], plp[r], plw[r], ps[r]};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] += __shfl_xor(v[q], o);
#pragma unroll
      for (int q = 0; q < (KL ? 4 : 1); ++q) d[q] += __shfl_xor(d[q], o);
    }
    const int i = ibase + r;
    if (lane == 0 && i < N) {
#pragma unroll
      for (int q = 0; q < 4; ++q) part[((int64_t)q * nsplit + split) * N + i] = v[q];
#pragma unroll
      for (int q = 0; q < (KL ? 4 : 1); ++q) dpart[((int64_t)q * nsplit + split) * N + i] = d[q];
    }
  }
}

// sum of the N x nsplit values of Z_i in float64: thread t takes elements t, t + 256, ...; folded by halving
__device__ __forceinline__ double tsne_fold_z(const double* __restrict__ dpart, int64_t n, double* sh) {
  double acc = 0.0;
  int64_t k = threadIdx.x;
  for (; k + 7 * TSNE_T < n; k += 8 * TSNE_T) {                  // eight loads in flight; the sum stays in ascending order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = dpart[k + u * TSNE_T];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; k < n; k += TSNE_T) acc += dpart[k];
  return slic_wg_fold<TSNE_T>(acc, sh);
}

// bpart[q][block]: q = 0 |gain grad|^2, 1 sum P log P, 2 sum P log w, 3 sum P; bpart[4][0] = Z
__global__ __launch_bounds__(TSNE_T) void tsne_update(const float* __restrict__ part, const double* __restrict__ dpart, int N, int nsplit,
                                                      int want_kl, float momentum, float lr,
                                                      float* __restrict__ Y, float* __restrict__ upd, float* __restrict__ gains,
                                                      float* __restrict__ grad_out, double* __restrict__ bpart) {
  __shared__ double sh[TSNE_T];
  const double Z = tsne_fold_z(dpart, (int64_t)N * nsplit, sh);
  const float zf = (float)Z;
  const int i = blockIdx.x * TSNE_T + threadIdx.x;
  double g2 = 0.0, kl[3] = {0.0, 0.0, 0.0};
  if (i < N) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int sp = 0; sp < nsplit; ++sp)
#pragma unroll
      for (int q = 0; q < 4; ++q) s[q] += part[((int64_t)q * nsplit + sp) * N + i];
    if (want_kl)
      for (int sp = 0; sp < nsplit; ++sp)
#pragma unroll
        for (int q = 0; q < 3; ++q) kl[q] += dpart[((int64_t)(q + 1) * nsplit + sp) * N + i];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float grad = 4.0f * (s[c] - s[2 + c] / zf);
      const int64_t at = 2 * (int64_t)i + c;
      if (grad_out) grad_out[at] = grad;
      const float u = upd[at];
      float g = gains[at];
      g = (u * grad < 0.0f) ? g + 0.2f : g * 0.8f;
      g = fmaxf(g, 0.01f);
      const float gg = grad * g;
      const float un = momentum * u - lr * gg;
      gains[at] = g;
      upd[at] = un;
      Y[at] += un;
      g2 += (double)gg * (double)gg;
    }
  }
  const double r0 = slic_wg_fold<TSNE_T>(g2, sh);
  if (threadIdx.x == 0) bpart[blockIdx.x] = r0;
  if (threadIdx.x == 0 && blockIdx.x == 0) bpart[4 * TSNE_MAX_BLOCKS] = Z;     // every workgroup holds the same bits
  if (want_kl) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double r = slic_wg_fold<TSNE_T>(kl[q], sh);
      if (threadIdx.x == 0) bpart[(q + 1) * TSNE_MAX_BLOCKS + blockIdx.x] = r;
    }
  }
}

__global__ __launch_bounds__(TSNE_T) void tsne_record(int nblocks, int want_kl, float exag, const double* __restrict__ bpart,
                                                      double* __restrict__ record) {
  __shared__ double sh[TSNE_T];
  const int t = threadIdx.x;
  const double Z = bpart[4 * TSNE_MAX_BLOCKS];
  double v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = slic_wg_fold<TSNE_T>((t < nblocks && (q == 0 || want_kl)) ? bpart[q * TSNE_MAX_BLOCKS + t] : 0.0, sh);
  if (t != 0) return;
  // KL of e P against Q = w / Z over the pairs i != j:  e (sum P log P + sum P (log e + log Z) - sum P log w)
  record[SLIC_TSNE_REC_Z] = Z;
  record[SLIC_TSNE_REC_KL] = want_kl ? (double)exag * (v[1] + v[3] * (log((double)exag) + log(Z)) - v[2]) : (double)NAN;
  record[SLIC_TSNE_REC_GRAD_NORM] = sqrt(v[0]);
  record[SLIC_TSNE_REC_SUM_P] = want_kl ? v[3] : (double)NAN;
}

// ---------------------------------------------------------------- centred Gram matrix (PCA)
// partial[s][a][b] = sum over the rows of share s, ascending, of (x_ia - mean_a)(x_ib - mean_b) in float64
__global__ __launch_bounds__(TSNE_T) void tsne_gram_part(const float* __restrict__ X, int64_t N, int D, int64_t ldx, const double* __restrict__ mean,
                                                         int S, double* __restrict__ partial) {
  __shared__ double A[64][17], B[64][17];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int a0 = blockIdx.y * 16, b0 = blockIdx.x * 16, s = blockIdx.z;
  const int64_t per = (N + S - 1) / S;
  const int64_t i0 = (int64_t)s * per, i1 = i0 + per < N ? i0 + per : N;
  double acc = 0.0;
  for (int64_t r0 = i0; r0 < i1; r0 += 64) {
    for (int e = tid; e < 64 * 16; e += TSNE_T) {
      const int r = e >> 4, c = e & 15;
      const int64_t i = r0 + r;
      A[r][c] = (i < i1 && a0 + c < D) ? (double)X[i * ldx + a0 + c] - mean[a0 + c] : 0.0;
      B[r][c] = (i < i1 && b0 + c < D) ? (double)X[i * ldx + b0 + c] - mean[b0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 64; ++r) acc = fma(A[r][ty], B[r][tx], acc);
    __syncthreads();
  }
  const int a = a0 + ty, b = b0 + tx;
  if (a < D && b < D) partial[((int64_t)s * D + a) * D + b] = acc;
}

__global__ __launch_bounds__(TSNE_T) void tsne_gram_fold(const double* __restrict__ partial, int D, int S, double* __restrict__ G) {
  const int64_t k = (int64_t)blockIdx.x * TSNE_T + threadIdx.x, n = (int64_t)D * D;
  if (k >= n) return;
  double acc = 0.0;
  for (int s = 0; s < S; ++s) acc += partial[(int64_t)s * n + k];
  G[k] = acc;
}

// ---------------------------------------------------------------- host side
struct TsneLayout {
  float* part;          // [4][TSNE_MAX_SPLIT][N]
  double* dpart;        // [4][TSNE_MAX_SPLIT][N]
  double* bpart;        // [4][TSNE_MAX_BLOCKS], then Z
  double* sum_part;     // [TSNE_G]
  double* total;        // [1]
};

static size_t tsne_layout(void* base, int64_t N, TsneLayout* L) {
  SlicCarver c(base);
  TsneLayout l;
  l.part = c.take<float>((size_t)4 * TSNE_MAX_SPLIT * (size_t)N);
  l.dpart = c.take<double>((size_t)4 * TSNE_MAX_SPLIT * (size_t)N);
  l.bpart = c.take<double>(4 * TSNE_MAX_BLOCKS + 1);
  l.sum_part = c.take<double>(TSNE_G);
  l.total = c.take<double>(1);
  if (L) *L = l;
  return c.off;
}

// column shares of the forces kernel: about eight workgroups per compute unit, every share at least 64 columns
static int tsne_splits(int64_t N, int cus) {
  const int64_t row_blocks = slic_cdiv(N, TSNE_FR);
  int64_t s = slic_cdiv(8 * (int64_t)cus, row_blocks);
  if (s > TSNE_MAX_SPLIT) s = TSNE_MAX_SPLIT;
  if (s > slic_cdiv(N, 64)) s = slic_cdiv(N, 64);
  return s < 1 ? 1 : (int)s;
}

extern "C" size_t slic_tsne_workspace_bytes(int64_t N) {
  if (!tsne_size_ok(N)) return 0;
  return tsne_layout(nullptr, N, nullptr);
}

extern "C" int slic_tsne_sqdist(const float* X, int64_t N, int D, int64_t ldx, float* d2, void* stream) {
  SLIC_REQUIRE(tsne_size_ok(N) && D >= 1, "slic_tsne_sqdist: N = %lld, D = %d (2 <= N <= %d, D >= 1)", (long long)N, D, SLIC_TSNE_MAX_N);
  SLIC_REQUIRE(X && d2 && ldx >= D, "slic_tsne_sqdist: NULL argument or ldx < D");
  const unsigned g = (unsigned)slic_cdiv(N, 64);
  tsne_sqdist<<<dim3(g, g), TSNE_T, 0, S_(stream)>>>(X, (int)N, D, ldx, d2);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_tsne_cond_p(float* P, int64_t N, double perplexity, float* beta, void* stream) {
  SLIC_REQUIRE(tsne_size_ok(N), "slic_tsne_cond_p: N = %lld (2 <= N <= %d)", (long long)N, SLIC_TSNE_MAX_N);
  SLIC_REQUIRE(P && beta && perplexity > 0.0, "slic_tsne_cond_p: NULL argument or perplexity <= 0");
  const size_t lds = (size_t)(N < TSNE_ROW_LDS ? N : TSNE_ROW_LDS) * sizeof(float);
  SLIC_LDS_LIMIT(tsne_cond_p, lds);
  tsne_cond_p<<<(unsigned)N, TSNE_T, lds, S_(stream)>>>(P, (int)N, log(perplexity), beta);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_tsne_symmetrize(float* P, int64_t N, void* workspace, void* stream) {
  SLIC_REQUIRE(tsne_size_ok(N), "slic_tsne_symmetrize: N = %lld (2 <= N <= %d)", (long long)N, SLIC_TSNE_MAX_N);
  SLIC_REQUIRE(P && workspace, "slic_tsne_symmetrize: NULL argument");
  TsneLayout L;
  tsne_layout(workspace, N, &L);
  hipStream_t st = S_(stream);
  tsne_sum_part<<<TSNE_G, TSNE_T, 0, st>>>(P, N * N, L.sum_part);
  SLIC_LAUNCH_CHECK();
  tsne_sum_fold<<<1, TSNE_T, 0, st>>>(L.sum_part, L.total);
  SLIC_LAUNCH_CHECK();
  const unsigned g = (unsigned)slic_cdiv(N, 32);
  tsne_sym_apply<<<dim3(g, g), TSNE_T, 0, st>>>(P, (int)N, L.total);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_tsne_step(const float* P, int64_t N, float exaggeration, float momentum, float learning_rate, int want_kl, float* Y,
                              float* update, float* gains, float* grad_out, double* record, void* workspace, void* stream) {
  SLIC_REQUIRE(tsne_size_ok(N), "slic_tsne_step: N = %lld (2 <= N <= %d)", (long long)N, SLIC_TSNE_MAX_N);
  SLIC_REQUIRE(P && Y && update && gains && record && workspace, "slic_tsne_step: NULL argument");
  const int cus = slic_device_cus();
  if (!cus) {
    slic_set_error("slic_tsne_step: cannot query the device's compute units");
    return SLIC_EHIP;
  }
  TsneLayout L;
  tsne_layout(workspace, N, &L);
  hipStream_t st = S_(stream);
  const int n = (int)N, nsplit = tsne_splits(N, cus), nblocks = (int)slic_cdiv(N, TSNE_T);
  const dim3 gf((unsigned)slic_cdiv(N, TSNE_FR), (unsigned)nsplit);
  if (want_kl) tsne_forces<true><<<gf, TSNE_T, 0, st>>>(P, Y, n, exaggeration, L.part, L.dpart);
  else tsne_forces<false><<<gf, TSNE_T, 0, st>>>(P, Y, n, exaggeration, L.part, L.dpart);
  SLIC_LAUNCH_CHECK();
  tsne_update<<<nblocks, TSNE_T, 0, st>>>(L.part, L.dpart, n, nsplit, want_kl, momentum, learning_rate, Y, update, gains, grad_out, L.bpart);
  SLIC_LAUNCH_CHECK();
  tsne_record<<<1, TSNE_T, 0, st>>>(nblocks, want_kl, exaggeration, L.bpart, record);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}

extern "C" int slic_tsne_gram(const float* X, int64_t N, int D, int64_t ldx, const double* mean, int shares, double* partial, double* G,
                              void* stream) {
  SLIC_REQUIRE(N >= 1 && D >= 1 && D <= SLIC_TSNE_GRAM_MAX_D && shares >= 1 && shares <= 65535, "slic_tsne_gram: N = %lld, D = %d, shares = %d",
               (long long)N, D, shares);
  SLIC_REQUIRE(X && mean && partial && G && ldx >= D, "slic_tsne_gram: NULL argument or ldx < D");
  const unsigned g = (unsigned)slic_cdiv(D, 16);
  tsne_gram_part<<<dim3(g, g, (unsigned)shares), TSNE_T, 0, S_(stream)>>>(X, N, D, ldx, mean, shares, partial);
  SLIC_LAUNCH_CHECK();
  tsne_gram_fold<<<(unsigned)slic_cdiv((int64_t)D * D, TSNE_T), TSNE_T, 0, S_(stream)>>>(partial, D, shares, G);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
