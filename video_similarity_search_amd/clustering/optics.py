"""
OPTICS with the cosine metric on the MI355X — drop-in for the reference's
    OPTICS(min_samples=3, max_eps=0.20, cluster_method='dbscan', metric='cosine', n_jobs=-1).fit(embeddings)   <- clustering/cluster_masks.py:88-89
with sklearn 1.7's labels and the reachability plot behind them (rules in include/slic_hip.h, slic_optics_cosine).  The whole fit is
one call into csrc/optics.hip: DBSCAN's label passes at eps = max_eps with OPTICS's border rule, core distances from the library's
top-k search, then every cluster's reachability walk at once (a cluster's walk touches its own rows only), so the dependent steps are
the largest cluster's rows, not N.  What OPTICS gives over DBSCAN is one fit and many cuts: cluster_optics_dbscan() cuts the same plot at
any eps <= max_eps in O(N) on the host, without another N x N pass.
Only metric='cosine', cluster_method='dbscan' and a finite max_eps (what the reference passes) are supported.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._device import require_device, resident_rows, sized_workspace

_STATS = ("band_rechecks", "walk_band_rechecks", "core_rows", "n_clusters", "largest_cluster", "walk_steps", "walk_launches",
          "host_loop_clusters", "ms_prep", "ms_count", "ms_compact", "ms_link", "ms_number", "ms_border", "ms_core_dist", "ms_walk")


class HipOpticsKernels:
    """the device side of OPTICS: resident rows and the one library call.  `OPTICS(kernels=)` takes another provider with the same two
    methods (tests of the host logic on a GPU-less machine pass a NumPy one as an ARGUMENT; the product has no other)."""

    def __init__(self):
        require_device("OPTICS")
        self.last_stats = None

    def resident(self, data):
        """fp32 device rows with unit column stride (no copy when they already are)"""
        return resident_rows(data, "OPTICS")

    def optics(self, rows, max_eps, min_samples, walk=True):
        """-> (labels int32 [N], is_core bool [N], core_dist float32 [N], reachability float32 [N], predecessor int32 [N],
        ordering int32 [N], n_clusters) as host arrays; walk=False: labels only, the four walk arrays are None"""
        N, D = rows.shape
        _lib.require_device(rows)
        ws = sized_workspace("slic_optics_cosine_workspace_bytes", (N, D, int(min_samples)), rows.device, "optics",
                             "OPTICS: {} x {} rows with min_samples = {} are outside what slic_optics_cosine takes (1 <= D <= 512, "
                             "2 <= min_samples <= min(N, 89), rows of int32 indices, < 4 GiB padded)".format(N, D, min_samples))
        dev = rows.device
        ints = torch.empty(3 * N + 1, dtype=torch.int32, device=dev)                 # labels, predecessor, ordering, n_clusters
        flt = torch.empty(2 * N, dtype=torch.float32, device=dev)                    # core distances, reachability
        core = torch.empty(N, dtype=torch.uint8, device=dev)
        labels, pred, order, ncl = ints[:N], ints[N:2 * N], ints[2 * N:3 * N], ints[3 * N:]
        cd, reach = flt[:N], flt[N:]
        call("slic_optics_cosine", ptr(rows), N, rows.stride(0), D, float(max_eps), int(min_samples), ptr(labels), ptr(core),
             ptr(cd) if walk else None, ptr(reach) if walk else None, ptr(pred) if walk else None, ptr(order) if walk else None,
             ptr(ncl), ptr(ws), stream())
        if not walk:
            ints[N:3 * N] = 0
        hi = ints.cpu().numpy()
        hcore = core.cpu().numpy().astype(bool)
        st = (ctypes.c_double * 16)()
        call("slic_optics_cosine_stats", ptr(ws), st, stream())
        self.last_stats = dict(zip(_STATS, list(st)))
        if not walk:
            return hi[:N].copy(), hcore, None, None, None, None, int(hi[3 * N])
        hf = flt.cpu().numpy()
        return hi[:N].copy(), hcore, hf[:N].copy(), hf[N:].copy(), hi[N:2 * N].copy(), hi[2 * N:3 * N].copy(), int(hi[3 * N])


def cluster_optics_dbscan(*, reachability, core_distances, ordering, eps):
    """sklearn.cluster.cluster_optics_dbscan: the DBSCAN-like cut of a reachability plot at eps (<= the fit's max_eps), O(N) on the
    host.  -> labels [N], -1 = noise"""
    reach = np.asarray(reachability)
    cd = np.asarray(core_distances)
    order = np.asarray(ordering)
    n = len(cd)
    labels = np.zeros(n, dtype=int)
    far = reach > eps
    near = cd <= eps
    labels[order] = np.cumsum(far[order] & near[order]) - 1
    labels[far & ~near] = -1
    return labels


class OPTICS:
    """sklearn-shaped: OPTICS(min_samples, max_eps, metric='cosine', cluster_method='dbscan', eps=None).fit(X) sets
        labels_          np.int32 [N], -1 = noise: the cut at eps (None: max_eps)
        ordering_        np.int32 [N], the walk's order
        reachability_    np.float32 [N], indexed by row (+inf for noise rows and every cluster's first row)
        core_distances_  np.float32 [N], +inf for non-core rows
        predecessor_     np.int32 [N], -1 where reachability_ is +inf
        n_clusters_      clusters of labels_ (noise not counted)
        stats_           the device call's counters (walk steps, launches, largest cluster, float64 rechecks, pass times)
    min_samples: an integer >= 2, or a float in (0, 1]: max(2, int(min_samples * N)).
    X: ndarray, CPU tensor, or device tensor (used in place)."""

    def __init__(self, min_samples=5, max_eps=np.inf, metric='cosine', cluster_method='dbscan', eps=None, kernels=None):
        self.min_samples = min_samples
        self.max_eps = max_eps
        self.metric = metric
        self.cluster_method = cluster_method
        self.eps = eps
        self.kernels = kernels

    def fit(self, X, y=None):
        if self.metric != 'cosine':
            raise NotImplementedError("OPTICS on the GPU supports metric='cosine' (what cluster_masks.py:89 passes), got "
                                      "{!r}".format(self.metric))
        if self.cluster_method != 'dbscan':
            raise NotImplementedError("OPTICS on the GPU supports cluster_method='dbscan' (what cluster_masks.py:89 passes): the "
                                      "'xi' extraction is not built, got {!r}".format(self.cluster_method))
        max_eps = float(self.max_eps)
        if math.isnan(max_eps) or max_eps < 0:
            raise ValueError("max_eps must be >= 0, got {!r}".format(self.max_eps))
        if not math.isfinite(max_eps):
            raise NotImplementedError("OPTICS on the GPU needs a finite max_eps: the device form searches a radius (the reference "
                                      "passes 0.20), got {!r}".format(self.max_eps))
        eps = max_eps if self.eps is None else float(self.eps)
        if eps > max_eps:
            raise ValueError("eps ({}) must be at most max_eps ({})".format(eps, max_eps))
        if not eps >= 0:
            raise ValueError("eps must be >= 0, got {!r}".format(self.eps))
        k = HipOpticsKernels() if self.kernels is None else self.kernels     # raises SlicError without a gfx950 device
        rows = k.resident(X)
        N = rows.shape[0]
        ms = self.min_samples
        if isinstance(ms, (float, np.floating)):
            if not 0 < ms <= 1:
                raise ValueError("min_samples must be an integer >= 2 or a float in (0, 1], got {!r}".format(ms))
            ms = max(2, int(ms * N))                                          # a fraction of the rows, as sklearn reads it
        elif int(ms) != ms or ms < 2:
            raise ValueError("min_samples must be an integer >= 2 or a float in (0, 1], got {!r}".format(ms))
        ms = int(ms)
        if ms > N:
            raise ValueError("min_samples ({}) must be no greater than the number of samples ({})".format(ms, N))
        labels, is_core, cd, reach, pred, order, n_clusters = k.optics(rows, max_eps, ms)
        self.ordering_ = np.asarray(order, dtype=np.int32)
        self.reachability_ = np.asarray(reach, dtype=np.float32)
        self.core_distances_ = np.asarray(cd, dtype=np.float32)
        self.predecessor_ = np.asarray(pred, dtype=np.int32)
        if eps < max_eps:
            labels = cluster_optics_dbscan(reachability=self.reachability_, core_distances=self.core_distances_,
                                           ordering=self.ordering_, eps=eps)
            n_clusters = int(labels.max()) + 1 if len(labels) else 0
        self.labels_ = np.asarray(labels, dtype=np.int32)
        self.n_clusters_ = int(n_clusters)
        self.stats_ = getattr(k, "last_stats", None)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
