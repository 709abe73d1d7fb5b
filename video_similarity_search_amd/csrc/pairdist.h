// The rowwise distance of models/triplet_net.py:29-33, shared by pair_distance_kernel (loss.hip) and triplet_val_batch_kernel
// (validate.hip) so that both give the same bits on the same rows: lane l of a wave accumulates elements l, l + 64, l + 128, ... of its
// row in that order, the 64 partial sums meet in an xor butterfly, lane 0's value is the result.
//   cosine   : 1 - x.y / (max(|x|, 1e-8) * max(|y|, 1e-8))        (F.cosine_similarity's per-norm clamp)
//   euclidean: || x - y + 1e-6 ||_2                                (F.pairwise_distance's eps, added to the difference)
#pragma once
#include "common.h"
#include <math.h>

// one element of the (x, y) pair: a = x.y (cosine) or the squared difference (euclidean); b = x.x, c = y.y (cosine only)
__device__ __forceinline__ void slic_pd_step(float x, float y, int euclid, float& a, float& b, float& c) {
  if (euclid) { const float d = x - y + 1e-6f; a = fmaf(d, d, a); }
  else { a = fmaf(x, y, a); b = fmaf(x, x, b); c = fmaf(y, y, c); }
}

__device__ __forceinline__ void slic_pd_wave_sum(float& a, float& b, float& c) {
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c += __shfl_xor(c, o); }
}

// from the wave-reduced sums
__device__ __forceinline__ float slic_pd_finish(float a, float b, float c, int euclid) {
  return euclid ? sqrtf(a) : 1.0f - a / (fmaxf(sqrtf(b), 1e-8f) * fmaxf(sqrtf(c), 1e-8f));
}
