// Dense ids of an arbitrary int32 labelling, shared by the NMI / AMI call (metrics.hip, where the kernels live) and the
// silhouette call (silhouette.hip): ids 0 .. U - 1 by ascending label value, class sizes, and — when asked for — the rows in
// (id, row) order, which the stable radix sort gives for free by carrying the row number along with the key.
#pragma once
#include "common.h"

#define SLIC_LABEL_CHUNK 64           // keys per thread in a radix pass (< 256: the packed counters are bytes)

struct SlicLabelScratch {
  uint32_t *keys_a, *keys_b;          // [N] each
  uint32_t* uniq;                     // [N] out: the distinct keys, ascending; label value = key ^ 0x80000000
  int* hist;                          // [16 * ceil(N / SLIC_LABEL_CHUNK)]
  int* pos;                           // [N]
  int* start;                         // [N] out: start[u] = first position of id u in the sorted order
  int *ord_a, *ord_b;                 // [N] each, or both NULL; out (ord_a): row numbers sorted by (id, row)
};

// every array of the scratch from a carver, in a fixed order (`order`: with ord_a / ord_b)
static inline void slic_label_scratch_take(SlicCarver& c, int64_t N, bool order, SlicLabelScratch* S) {
  const size_t n = (size_t)N, T = (size_t)slic_cdiv(N, SLIC_LABEL_CHUNK);
  S->keys_a = c.take<uint32_t>(n);
  S->keys_b = c.take<uint32_t>(n);
  S->uniq = c.take<uint32_t>(n);
  S->hist = c.take<int>(16 * T);
  S->pos = c.take<int>(n);
  S->start = c.take<int>(n);
  S->ord_a = order ? c.take<int>(n) : nullptr;
  S->ord_b = order ? c.take<int>(n) : nullptr;
}

// ids[N], cnt[N] (the first U entries are written) and *n_uniq = U, all on the device; no host synchronisation
int slic_label_dense_ids(const int32_t* labels, int n, const SlicLabelScratch& S, int* ids, int* cnt, int* n_uniq, hipStream_t st);
