"""
DBSCAN with the cosine metric on the MI355X — drop-in for the reference's
    DBSCAN(eps=0.14, min_samples=2, metric='cosine', n_jobs=-1).fit(embeddings)        <- clustering/cluster_masks.py:55-61
with sklearn 1.7's labels (rules in include/slic_hip.h, slic_dbscan_cosine).  The whole fit is one call into
csrc/dbscan.hip: neighbour counts from a fused similarity GEMM over the upper triangle of tiles, core rows compacted,
connected components of the cores by union-find on the device, border rows labelled by a third GEMM pass.  The N x N
distance matrix is neither written nor copied to the host; what comes back is N labels, N core flags and N counts.
Only metric='cosine' (what the reference passes) is supported.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._device import require_device, resident_rows, sized_workspace

_STATS = ("band_rechecks", "skipped_tiles", "core_rows", "border_candidates", "ms_prep", "ms_count", "ms_compact", "ms_link", "ms_number",
          "ms_border")


class HipDbscanKernels:
    """the device side of DBSCAN: resident rows and the one library call.  `DBSCAN(kernels=)` takes another provider with the
    same two methods (tests of the host logic on a GPU-less machine pass a NumPy one as an ARGUMENT; the product has no other)."""

    def __init__(self):
        require_device("DBSCAN")
        self.last_stats = None

    def resident(self, data):
        """fp32 device rows with unit column stride (no copy when they already are)"""
        return resident_rows(data, "DBSCAN")

    def dbscan(self, rows, eps, min_samples):
        """-> (labels int32 [N], is_core bool [N], counts int32 [N], n_clusters) as host arrays"""
        N, D = rows.shape
        _lib.require_device(rows)
        ws = sized_workspace("slic_dbscan_cosine_workspace_bytes", (N, D), rows.device, "dbscan",
                             "DBSCAN: {} x {} rows are outside what slic_dbscan_cosine takes (1 <= D <= 512, rows of int32 indices, "
                             "< 4 GiB padded)".format(N, D))
        labels = torch.empty(N, dtype=torch.int32, device=rows.device)
        core = torch.empty(N, dtype=torch.uint8, device=rows.device)
        counts = torch.empty(N, dtype=torch.int32, device=rows.device)
        ncl = torch.empty(1, dtype=torch.int32, device=rows.device)
        call("slic_dbscan_cosine", ptr(rows), N, rows.stride(0), D, float(eps), int(min_samples), ptr(labels), ptr(core),
             ptr(counts), ptr(ncl), ptr(ws), stream())
        out = torch.cat([labels, core.to(torch.int32), counts, ncl]).cpu().numpy()
        st = (ctypes.c_double * len(_STATS))()
        call("slic_dbscan_cosine_stats", ptr(ws), st, stream())
        self.last_stats = dict(zip(_STATS, list(st)))
        return out[:N], out[N:2 * N].astype(bool), out[2 * N:3 * N], int(out[3 * N])


class DBSCAN:
    """sklearn-shaped: DBSCAN(eps, min_samples, metric='cosine').fit(X) sets
        labels_              np.int32 [N], -1 = noise
        core_sample_indices_ np.int64, ascending
        n_clusters_          number of clusters (noise not counted)
        n_neighbors_         np.int32 [N], |N(i)| with the row itself (not in sklearn; what the core test reads)
    X: ndarray, CPU tensor, or device tensor (used in place)."""

    def __init__(self, eps=0.5, min_samples=5, metric='cosine', kernels=None):
        self.eps = eps
        self.min_samples = min_samples
        self.metric = metric
        self.kernels = kernels

    def fit(self, X, y=None):
        if self.metric != 'cosine':
            raise NotImplementedError("DBSCAN on the GPU supports metric='cosine' (what cluster_masks.py:58 passes), got "
                                      "{!r}".format(self.metric))
        if not self.eps >= 0:
            raise ValueError("eps must be >= 0, got {!r}".format(self.eps))
        if int(self.min_samples) != self.min_samples or self.min_samples < 1:
            raise ValueError("min_samples must be an integer >= 1, got {!r}".format(self.min_samples))
        k = HipDbscanKernels() if self.kernels is None else self.kernels     # raises SlicError without a gfx950 device
        rows = k.resident(X)
        if rows.shape[0] < 1:
            raise ValueError("DBSCAN needs at least one row")
        labels, is_core, counts, n_clusters = k.dbscan(rows, float(self.eps), int(self.min_samples))
        self.labels_ = np.asarray(labels, dtype=np.int32)
        self.core_sample_indices_ = np.flatnonzero(np.asarray(is_core)).astype(np.int64)
        self.n_neighbors_ = np.asarray(counts, dtype=np.int32)
        self.n_clusters_ = int(n_clusters)
        self.stats_ = getattr(k, "last_stats", None)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_
