"""TEST-ONLY kernel provider for DBSCAN(kernels=...) and the float64 oracle of the GPU tests: the rules of slic_dbscan_cosine
(include/slic_hip.h) written out directly in NumPy, O(N^2) work in row chunks (N up to a few ten thousand).  Never shipped, never
imported by the package."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from host_rows import host_rows


def inv_norms(X):
    """float64 1 / ||x|| of every row, 0 for a zero row"""
    n = np.sqrt(np.einsum("ij,ij->i", X, X))
    out = np.zeros_like(n)
    np.divide(1.0, n, out=out, where=n > 0)
    return out


def distance_chunks(X, chunk=512):
    """yields (s, d) with d = the float64 distances of rows s .. s + len(d) to every row, d(i, i) = 0 (rule 1)"""
    X64 = np.asarray(X, dtype=np.float64)
    inv = inv_norms(X64)
    for s in range(0, len(X64), chunk):
        g = X64[s:s + chunk] @ X64.T
        d = np.clip(1.0 - (g * inv[s:s + chunk, None]) * inv[None, :], 0.0, 2.0)
        d[np.arange(len(d)), s + np.arange(len(d))] = 0.0
        yield s, d


def dbscan_fp64(X, eps, min_samples, chunk=512):
    """-> (labels int32 [N], is_core bool [N], counts int32 [N], n_clusters) by rules 1-5"""
    X = np.asarray(X, dtype=np.float32)
    N = len(X)
    counts = np.zeros(N, np.int64)
    for s, d in distance_chunks(X, chunk):
        counts[s:s + len(d)] = (d <= eps).sum(axis=1)
    core = counts >= min_samples
    cidx = np.flatnonzero(core)
    pos = np.full(N, -1, np.int64)
    pos[cidx] = np.arange(len(cidx))
    ea, eb = [], []
    border_rows = np.flatnonzero(~core & (counts >= 2))
    for s, d in distance_chunks(X[cidx], chunk) if len(cidx) else ():
        a, b = np.nonzero(d <= eps)
        keep = a + s < b
        ea.append(a[keep] + s)
        eb.append(b[keep])
    labels = np.full(N, -1, np.int64)
    ncl = 0
    if len(cidx):
        a = np.concatenate(ea) if ea else np.zeros(0, np.int64)
        b = np.concatenate(eb) if eb else np.zeros(0, np.int64)
        g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(len(cidx), len(cidx)))
        ncl, comp = connected_components(g, directed=False)
        # renumber by smallest member (connected_components already numbers in order of first appearance = smallest index)
        first = np.full(ncl, len(cidx), np.int64)
        np.minimum.at(first, comp, np.arange(len(cidx)))
        order = np.argsort(first, kind="stable")
        rank = np.empty(ncl, np.int64)
        rank[order] = np.arange(ncl)
        labels[cidx] = rank[comp]
        if len(border_rows):
            X64 = np.asarray(X, dtype=np.float64)
            inv = inv_norms(X64)
            C = X64[cidx]
            for s in range(0, len(border_rows), chunk):
                rows = border_rows[s:s + chunk]
                gm = X64[rows] @ C.T
                d = np.clip(1.0 - (gm * inv[rows, None]) * inv[None, cidx], 0.0, 2.0)
                lab = np.where(d <= eps, labels[cidx][None, :], np.iinfo(np.int64).max).min(axis=1)
                labels[rows] = np.where(lab == np.iinfo(np.int64).max, -1, lab)
    return labels.astype(np.int32), core, counts.astype(np.int32), int(ncl)


class NumpyDbscanKernels:
    """the HipDbscanKernels interface on host arrays"""

    def __init__(self):
        self.last_stats = None

    def resident(self, data):
        return host_rows(data, "DBSCAN")

    def dbscan(self, rows, eps, min_samples):
        return dbscan_fp64(rows, eps, min_samples)
