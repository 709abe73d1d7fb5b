"""
Average-linkage agglomerative clustering with the cosine metric, cut by a distance threshold, on the MI355X — for the reference's
    AgglomerativeClustering(n_clusters=None, linkage='average', distance_threshold=0.24, affinity='cosine').fit(embeddings)
                                                                                        <- clustering/cluster_masks.py:49-54
(sklearn >= 1.4 spells the last argument metric='cosine').

No N x N matrix.  On L2-normalised rows the average of all pairwise cosine distances between clusters A and B is
    d(A, B) = 1 - (S_A . S_B) / (|A| |B|),     S_A = the plain sum of A's unit rows,
so a cluster is one D-vector and a count, a merge is a vector add, and the nearest cluster of a cluster is an inner-product nearest
neighbour search over the means M = S / n: the fused similarity GEMM + top-k kernel (csrc/topk.hip) that FINCH already uses.

No N dependent merges.  Average linkage is reducible, d(k, i u j) >= min(d(k, i), d(k, j)), so two clusters that are each other's nearest
neighbour (a reciprocal pair) are a merge of the greedy dendrogram whatever happens elsewhere, and all reciprocal pairs below the
threshold merge in the same round.  The globally closest pair is always reciprocal, so the rounds end exactly at the greedy result: the
partition in which no two clusters are closer than the threshold.  By the same inequality a cluster's cached nearest neighbour stays
valid until that neighbour takes part in a merge: after the first round only those "stale" clusters search again (n_query_rows_).

Distances are fp32 (the search's clip(1 - q . g, 0, 2) on fp32 means of fp32 sums); a merge height within ~D * 6e-8 of the threshold may
fall on either side of it, where sklearn's float64 condensed matrix decides differently.  Exactly tied rows (duplicates) form a star
under the search's lowest-index tie-breaking: a group of m identical rows takes m - 1 rounds, each of them tiny.

`labels_` is the same PARTITION as sklearn's, not sklearn's label numbers (its _hc_cut numbers clusters from the node ids of the full
tree above the cut): clusters are numbered 0 .. C-1 in ascending order of their smallest row, i.e. in order of first appearance.
Out of scope: n_clusters (a parallel round can overshoot a count), other linkages and metrics, children_ and distances_.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._device import require_device, resident_rows, workspace_bytes


class HipAggloKernels:
    """the device side: the state of one run in a workspace of csrc/agglo.hip and the four library calls.  `AgglomerativeClustering(kernels=)`
    takes another provider with the same methods (tests of the host logic on a GPU-less machine pass a NumPy one as an ARGUMENT; the
    product has no other)."""

    def __init__(self):
        require_device("AgglomerativeClustering")

    def resident(self, data):
        """fp32 device rows with unit column stride (no copy when they already are)"""
        return resident_rows(data, "AgglomerativeClustering")

    def start(self, rows):
        """every row a cluster of its own; -> the number of rows that cannot be normalised (zero norm or a non-finite value)"""
        N, D = rows.shape
        _lib.require_device(rows)
        nbytes = workspace_bytes("slic_agglo_workspace_bytes", (N, D),
                                 "AgglomerativeClustering: {} x {} rows are outside what slic_agglo_start takes (1 <= D <= 512, "
                                 "N <= 2^24, < 4 GiB padded)".format(N, D))
        self.N, self.D, self.A, self.Q = N, D, N, N
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=rows.device)
        self.rec = (ctypes.c_int64 * 5)()                 # SLIC_AGGLO_RECORD
        self.search_ns = 0                                 # device time of the searches, summed, when SLIC_AGGLO_TIMING=1
        bad = ctypes.c_int32(0)
        call("slic_agglo_start", ptr(rows), N, rows.stride(0), D, ptr(self.ws), ctypes.byref(bad), stream())
        return int(bad.value)

    def _record(self):
        merged, self.A, self.Q, key, ns = (int(v) for v in self.rec)
        self.search_ns += max(ns, 0)
        dmin = np.array([(key >> 32) & 0xFFFFFFFF], np.uint32).view(np.float32)[0]
        return merged, self.A, self.Q, float(dmin)

    def round(self, threshold):
        """search the stale clusters, merge the reciprocal pairs below the threshold -> (pairs merged, live clusters, stale clusters,
        smallest nearest-cluster distance among the clusters that were live before the merges)"""
        tws = _lib.workspace(_lib.load().slic_cosine_topk_workspace_bytes(self.Q, self.A, 2), self.ws.device, "agglo_topk")
        call("slic_agglo_round", ptr(self.ws), self.N, self.D, self.A, self.Q, float(threshold), ptr(tws), self.rec, stream())
        return self._record()

    def merge_closest(self):
        """after a round that merged nothing: merge the closest cluster (lowest distance, then lowest id) with its nearest cluster
        -> (pairs merged, live clusters, stale clusters)"""
        call("slic_agglo_merge_closest", ptr(self.ws), self.N, self.D, self.rec, stream())
        return self._record()[:3]

    def labels(self):
        """np.int32 [N]: clusters numbered by their smallest row"""
        out = torch.empty(self.N, dtype=torch.int32, device=self.ws.device)
        call("slic_agglo_labels", ptr(self.ws), self.N, self.D, ptr(out), stream())
        return out.cpu().numpy()


class AgglomerativeClustering:
    """sklearn-shaped: AgglomerativeClustering(n_clusters=None, metric='cosine', linkage='average', distance_threshold=t).fit(X) sets
        labels_         np.int32 [N]: sklearn's partition, clusters numbered 0 .. C-1 by their smallest row (NOT sklearn's numbers)
        n_clusters_     C
        n_leaves_       N
        rounds_         search-and-merge rounds run
        n_query_rows_   rows searched over all rounds (the sum of the stale counts: rounds_ * live clusters without the cache)
    Two clusters merge while their average cosine distance is < distance_threshold (sklearn: "at or above which clusters will not be
    merged").  affinity='cosine' is accepted as the old spelling of metric.  X: ndarray, CPU tensor, or device tensor (used in place)."""

    def __init__(self, n_clusters=None, *, metric='cosine', linkage='average', distance_threshold=None, affinity=None, kernels=None):
        self.n_clusters = n_clusters
        self.metric = metric
        self.linkage = linkage
        self.distance_threshold = distance_threshold
        self.affinity = affinity
        self.kernels = kernels

    def fit(self, X, y=None):
        metric = self.metric if self.affinity is None else self.affinity
        if metric != 'cosine':
            raise NotImplementedError("AgglomerativeClustering on the GPU supports metric='cosine' (what cluster_masks.py:53 passes): the "
                                      "cluster-sum identity behind it holds for cosine distances of unit rows only; got {!r}".format(metric))
        if self.linkage != 'average':
            raise NotImplementedError("AgglomerativeClustering on the GPU supports linkage='average' (what cluster_masks.py:51 passes): "
                                      "other linkages are not a function of cluster sums; got {!r}".format(self.linkage))
        if self.n_clusters is not None:
            raise NotImplementedError("AgglomerativeClustering on the GPU cuts by distance_threshold only (n_clusters=None, as "
                                      "cluster_masks.py:50 passes): a round merges many pairs at once and can overshoot a cluster count")
        if self.distance_threshold is None:
            raise ValueError("distance_threshold is required (n_clusters=None); the reference passes 0.24")
        t = float(self.distance_threshold)
        if not t >= 0:
            raise ValueError("distance_threshold must be >= 0, got {!r}".format(self.distance_threshold))
        k = HipAggloKernels() if self.kernels is None else self.kernels     # raises SlicError without a gfx950 device
        rows = k.resident(X)
        N = rows.shape[0]
        if N < 1:
            raise ValueError("AgglomerativeClustering needs at least one row")
        self.n_leaves_ = N
        self.rounds_ = self.n_query_rows_ = self.n_fallback_merges_ = 0
        if N == 1:                                  # nothing to search: no launch
            if not np.isfinite(_host(rows)).all() or not np.any(_host(rows)):
                raise ValueError("AgglomerativeClustering: the row has zero norm or a non-finite value")
            self.labels_, self.n_clusters_ = np.zeros(1, np.int32), 1
            return self
        bad = k.start(rows)
        if bad:
            raise ValueError("AgglomerativeClustering: {} row(s) have zero norm or a non-finite value; the cosine distance is "
                             "undefined for them".format(bad))
        live, stale = N, N
        while live > 1:
            self.rounds_ += 1
            self.n_query_rows_ += stale
            merged, live, stale, dmin = k.round(t)
            if merged == 0:
                if not dmin < t:
                    break                           # no two clusters are closer than the threshold: the greedy result
                # exact or last-bit ties can leave a round without a reciprocal pair; the closest pair is a greedy merge all the same
                merged, live, stale = k.merge_closest()
                self.n_fallback_merges_ += merged
                if merged == 0:
                    raise _lib.SlicError("AgglomerativeClustering: no pair to merge at nearest distance {} < {}".format(dmin, t))
        self.labels_ = np.asarray(k.labels(), dtype=np.int32)
        self.n_clusters_ = int(live)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_


def _host(rows):
    return rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
