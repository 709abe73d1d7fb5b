// Segment means of rows (the reference's coclr_classify.py:575, 622 `F.softmax(logit, -1).mean(0)` then `stack().mean(0)`, and :734
// `feature.mean(0)`): the R rows of x fall into V consecutive segments; segment v adds w[v] * sum of f(row) into one row of a table,
// f the identity (mode 0) or the softmax over the C columns (mode 1).
//
//   segment_mean_kernel : one workgroup of four waves per segment.  The rows are walked in chunks of SEG_CHUNK.  Mode 1, step A: wave
//                         q takes rows q, q + 4, ... of the chunk, strided over the C logits as softmax_ce_fwd_kernel is — pass 1 the
//                         row maximum, pass 2 sum expf(x - max), both finished by xor shuffles — and leaves (max, sum) in LDS.  Step B,
//                         after the barrier: thread t owns columns t, t + 256, ... (at most 16 at C <= 4096) and adds
//                         expf(x - max) / sum of every row of the chunk to its registers in ASCENDING row order, the rounding error
//                         of each addition collected beside the sum (seg_add).  So each output is one sequential compensated fp32
//                         sum over the rows of its segment, whatever the segment length and the wave that took the statistics: no
//                         atomics, no order left to scheduling, two runs give the same bits.  Mode 0 is step B alone.
//                         The three reads of a row come from L2; the whole input of a call is a few hundred KiB.
//
// A -inf logit beside a finite maximum gives expf(-inf) = 0; everything else non-finite (a row of -inf, a +inf, a NaN) comes out as
// IEEE arithmetic makes it: NaN in that segment's row of the table.  Compiled with -ffp-contract=off: w * acc is rounded before it is
// added to the table, as tests/segmean_cpu_kernels.py mirrors it.
#include "common.h"
#include <math.h>
#include <algorithm>
#include <vector>

#define SEG_CHUNK 64
#define SEG_MAX_C 4096
#define SEG_COLS (SEG_MAX_C / 256)

// sum += v with the rounding error of the addition kept in comp (Neumaier's form of compensated summation: exact error term whichever
// of the two is larger).  The segment's total is sum + comp: the correctly rounded sum to within an ulp however long the segment.
__device__ __forceinline__ void seg_add(float& sum, float& comp, float v) {
  const float t = sum + v;
  comp += fabsf(sum) >= fabsf(v) ? (sum - t) + v : (v - t) + sum;
  sum = t;
}

__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ x, int64_t ld, int C, const int32_t* __restrict__ seg_off,
                                                           const int32_t* __restrict__ rows, const float* __restrict__ w,
                                                           float* __restrict__ table, int64_t ldt, int mode, int accumulate) {
  __shared__ float s_max[SEG_CHUNK], s_sum[SEG_CHUNK];
  const int v = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r0 = seg_off[v], r1 = seg_off[v + 1];
  float acc[SEG_COLS], comp[SEG_COLS];
#pragma unroll
  for (int c = 0; c < SEG_COLS; ++c) acc[c] = comp[c] = 0.f;
  for (int base = r0; base < r1; base += SEG_CHUNK) {
    const int n = min(SEG_CHUNK, r1 - base);
    if (mode == 1) {
      for (int i = wave; i < n; i += 4) {
        const float* r = x + (int64_t)(base + i) * ld;
        float m = -INFINITY;
        for (int j = lane; j < C; j += 64) m = fmaxf(m, r[j]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float s = 0.f;
        for (int j = lane; j < C; j += 64) s += expf(r[j] - m);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) { s_max[i] = m; s_sum[i] = s; }
      }
      __syncthreads();
    }
    for (int i = 0; i < n; ++i) {
      const float* r = x + (int64_t)(base + i) * ld;
      if (mode == 1) {
        const float m = s_max[i], s = s_sum[i];
#pragma unroll
        for (int c = 0; c < SEG_COLS; ++c) {
          const int j = t + c * 256;
          if (j < C) seg_add(acc[c], comp[c], expf(r[j] - m) / s);
        }
      } else {
#pragma unroll
        for (int c = 0; c < SEG_COLS; ++c) {
          const int j = t + c * 256;
          if (j < C) seg_add(acc[c], comp[c], r[j]);
        }
      }
    }
    if (mode == 1) __syncthreads();          // the next chunk's statistics overwrite s_max / s_sum
  }
  const float wv = w[v];
  float* out = table + (int64_t)rows[v] * ldt;
#pragma unroll
  for (int c = 0; c < SEG_COLS; ++c) {
    const int j = t + c * 256;
    if (j < C) {
      const float y = wv * (isfinite(comp[c]) ? acc[c] + comp[c] : acc[c]);
      out[j] = accumulate ? out[j] + y : y;
    }
  }
}

extern "C" int slic_segment_mean(const float* x, int64_t ld, int R, int C, const void* segs, const void* segs_host, int V, int mode,
                                 int accumulate, float* table, int64_t ldt, int table_rows, void* stream) {
  SLIC_REQUIRE(x && segs && segs_host && table, "slic_segment_mean: null pointer");
  SLIC_REQUIRE(R >= 1 && V >= 1 && table_rows >= 1, "slic_segment_mean: R, V and table_rows must be at least 1");
  SLIC_REQUIRE(C >= 1 && C <= SEG_MAX_C, "slic_segment_mean: C = %d outside [1, %d]", C, SEG_MAX_C);
  SLIC_REQUIRE(ld >= (int64_t)C && ldt >= (int64_t)C, "slic_segment_mean: row pitches (%lld, %lld) must be at least C = %d",
               (long long)ld, (long long)ldt, C);
  SLIC_REQUIRE(mode == 0 || mode == 1, "slic_segment_mean: mode %d (0 = rows, 1 = softmax of the rows)", mode);
  SLIC_REQUIRE(accumulate == 0 || accumulate == 1, "slic_segment_mean: accumulate must be 0 or 1");
  const int32_t* off = (const int32_t*)segs_host;
  const int32_t* rows = off + (V + 1);
  SLIC_REQUIRE(off[0] >= 0 && off[V] <= R, "slic_segment_mean: segment offsets [%d, %d] leave the %d rows", off[0], off[V], R);
  for (int v = 0; v < V; ++v) {
    SLIC_REQUIRE(off[v + 1] >= off[v], "slic_segment_mean: segment offsets not ascending at segment %d", v);
    SLIC_REQUIRE(off[v + 1] > off[v], "slic_segment_mean: segment %d is empty", v);
    SLIC_REQUIRE(rows[v] >= 0 && rows[v] < table_rows, "slic_segment_mean: segment %d addresses row %d of a table of %d", v, rows[v],
                 table_rows);
  }
  std::vector<int32_t> sorted(rows, rows + V);
  std::sort(sorted.begin(), sorted.end());
  for (int v = 1; v < V; ++v)
    SLIC_REQUIRE(sorted[v] != sorted[v - 1], "slic_segment_mean: table row %d is addressed by two segments of one call", sorted[v]);
  const int32_t* d_off = (const int32_t*)segs;
  segment_mean_kernel<<<dim3((unsigned)V), dim3(256), 0, S_(stream)>>>(x, ld, C, d_off, d_off + (V + 1), (const float*)(d_off + 2 * V + 1),
                                                                       table, ldt, mode, accumulate);
  SLIC_LAUNCH_CHECK();
  return SLIC_OK;
}
