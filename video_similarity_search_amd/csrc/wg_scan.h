// One-workgroup scans and the fixed-order fold that the cluster step's kernels share (dbscan.hip, optics.hip, agglo.hip, metrics.hip,
// silhouette.hip).  T is the workgroup's size; every thread of the workgroup calls.
#pragma once
#include "common.h"

// thread t of T owns the run [*beg, *end) of ceil(n / T) consecutive elements of [0, n); the runs tile [0, n), trailing ones are empty
__host__ __device__ inline void slic_run_bounds(int n, int T, int t, int* beg, int* end) {
  const int per = (n + T - 1) / T;
  const int64_t b = (int64_t)t * per;
  *beg = b < n ? (int)b : n;
  *end = n - *beg < per ? n : *beg + per;
}

// exclusive scan of NV ints per thread: v[q] becomes the sum of the v[q] of the threads below, total[q] the workgroup's sum.  The
// __shfl_up ladder inside a wave, one wave total per value through sh (NV * (T / 64) ints).
template <int T, int NV>
__device__ __forceinline__ void slic_wg_scan(int (&v)[NV], int* sh, int (&total)[NV]) {
  static_assert(T % 64 == 0, "whole waves");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc[NV];                                                  // inclusive within the wave
#pragma unroll
  for (int q = 0; q < NV; ++q) inc[q] = v[q];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int u = __shfl_up(inc[q], o);
      if (lane >= o) inc[q] += u;
    }
  }
  __syncthreads();                                              // a previous call's readers are done with sh
  if (lane == 63) {
#pragma unroll
    for (int q = 0; q < NV; ++q) sh[q * (T / 64) + w] = inc[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    int below = 0, all = 0;
#pragma unroll
    for (int i = 0; i < T / 64; ++i) {
      const int x = sh[q * (T / 64) + i];
      if (i < w) below += x;
      all += x;
    }
    v[q] = below + inc[q] - v[q];
    total[q] = all;
  }
}

// exclusive scan of data[0 .. n) in place, in a fixed order: thread t adds its run (slic_run_bounds) in ascending order from 0; the T run
// sums are scanned by doubling (s[t] += s[t - o], o = 1 .. T / 2); a run's elements are then re-added in ascending order onto the sum of
// the runs before it.  *total (optional) = the sum.
template <int T, typename V>
__device__ __forceinline__ void slic_wg_scan_array(V* __restrict__ data, int n, V* __restrict__ total) {
  __shared__ V s[T];
  const int t = threadIdx.x;
  int lo, hi;
  slic_run_bounds(n, T, t, &lo, &hi);
  V sum = 0;
  for (int k = lo; k < hi; ++k) sum += data[k];
  s[t] = sum;
  __syncthreads();
  for (int o = 1; o < T; o <<= 1) {
    const V v = t >= o ? s[t - o] : (V)0;
    __syncthreads();
    if (t >= o) s[t] += v;
    __syncthreads();
  }
  V run = t > 0 ? s[t - 1] : (V)0;
  for (int k = lo; k < hi; ++k) {
    const V v = data[k];
    data[k] = run;
    run += v;
  }
  if (t == T - 1 && total) *total = s[T - 1];
}

// the workgroup's T values folded by halving (s[t] += s[t + o], o = T / 2 .. 1) through s (T doubles); every thread gets the sum
template <int T>
__device__ __forceinline__ double slic_wg_fold(double v, double* s) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int o = T / 2; o > 0; o >>= 1) {
    if (t < o) s[t] += s[t + o];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}
