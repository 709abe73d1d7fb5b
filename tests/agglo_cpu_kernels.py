"""TEST-ONLY kernel provider for AgglomerativeClustering(kernels=...) and the float64 oracle of the GPU tests: the rounds of
csrc/agglo.hip (include/slic_hip.h, slic_agglo_*) written out in NumPy — cluster sums and counts, a top-2 search of the stale clusters'
means against all live means, reciprocal pairs below the threshold merged at once.  Never shipped, never imported by the package."""
import os

import numpy as np

from host_rows import host_rows


def golden_cases():
    """(name, X, t, canonical labels) of every case of tests/golden/agglomerative.npz"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agglomerative.npz"))
    names = sorted({k.split("__")[0] for k in z.files})
    return [(n, z[n + "__X"], float(z[n + "__t"]), z[n + "__labels"]) for n in names]


def canonical(labels):
    """renumber any labelling 0 .. C-1 in order of first appearance (= by the smallest member of every cluster)"""
    labels = np.asarray(labels)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32)


class NumpyAggloKernels:
    """the HipAggloKernels interface on host arrays, in `dtype` arithmetic (float32: the device's semantics; float64: the oracle).
    heights collects the distance of every merge."""

    def __init__(self, dtype=np.float32, chunk=1024):
        self.dtype = dtype
        self.chunk = chunk
        self.heights = []

    def resident(self, data):
        return host_rows(data, "AgglomerativeClustering")

    def start(self, rows):
        x = rows.astype(np.float64)
        sq = np.einsum("ij,ij->i", x, x)
        bad = ~((sq > 0) & np.isfinite(sq))
        if bad.any():
            return int(bad.sum())
        N = len(x)
        self.N = N
        self.S = (x / np.sqrt(sq)[:, None]).astype(self.dtype)
        self.cnt = np.ones(N, np.int64)
        self.live = np.ones(N, bool)
        self.stale = np.ones(N, bool)
        self.nn = np.full(N, -1, np.int64)
        self.nd = np.full(N, np.inf, self.dtype)
        self.parent = np.arange(N)
        self.closest = -1
        self.heights = []
        return 0

    def search(self, Mq, M, own):
        """(position, distance) of the nearest row of M to every row of Mq other than position own[i]; ties -> lower position"""
        pos = np.empty(len(Mq), np.int64)
        dist = np.empty(len(Mq), self.dtype)
        for s in range(0, len(Mq), self.chunk):
            d = np.clip(1 - Mq[s:s + self.chunk] @ M.T, 0, 2).astype(self.dtype)
            r = np.arange(len(d))
            d[r, own[s:s + self.chunk]] = np.inf
            pos[s:s + self.chunk] = d.argmin(axis=1)
            dist[s:s + self.chunk] = d[r, pos[s:s + self.chunk]]
        return pos, dist

    def _merge(self, a, b):
        self.heights.extend(float(v) for v in self.nd[a])
        self.S[a] += self.S[b]
        self.cnt[a] += self.cnt[b]
        self.live[b] = False
        self.parent[b] = a
        lead = np.zeros(self.N, bool)
        lead[a] = True
        nn = np.where(self.nn >= 0, self.nn, 0)
        self.stale = self.live & (lead | (self.nn < 0) | ~self.live[nn] | lead[nn])
        return len(a), int(self.live.sum()), int(self.stale.sum())

    def round(self, threshold):
        act = np.flatnonzero(self.live)
        q = np.flatnonzero(self.stale)
        if len(q):
            pos = np.full(self.N, -1, np.int64)
            pos[act] = np.arange(len(act))
            M = (self.S[act] / self.cnt[act, None].astype(self.dtype)).astype(self.dtype)
            p, d = self.search(M[pos[q]], M, pos[q])
            self.nn[q], self.nd[q] = act[p], d
        nd = np.where(self.live, self.nd, np.inf)
        self.closest = int(np.lexsort((np.arange(self.N), nd))[0])
        dmin = float(nd[self.closest])
        a = act[(self.nn[self.nn[act]] == act) & (act < self.nn[act]) & (self.nd[act] < self.dtype(threshold))]
        merged, live, stale = self._merge(a, self.nn[a])
        return merged, live, stale, dmin

    def merge_closest(self):
        i = self.closest
        j = int(self.nn[i])
        a, b = min(i, j), max(i, j)
        self.nn[a] = b
        self.nd[a] = self.nd[i]
        return self._merge(np.array([a]), np.array([b]))

    def labels(self):
        root = self.parent.copy()
        while True:
            nxt = root[root]
            if np.array_equal(nxt, root):
                break
            root = nxt
        rank = np.cumsum(self.live) - 1
        return rank[root].astype(np.int32)


def agglo_fp64(X, t):
    """-> (canonical labels int32 [N], merge heights float64 [merges], the smallest nearest-cluster distance left at the end — inf when one
    cluster is left) of average-linkage / cosine clustering cut at t: the round algorithm in float64, run by the product's host loop"""
    from video_similarity_search_amd.clustering.agglomerative import AgglomerativeClustering
    k = NumpyAggloKernels(np.float64)
    m = AgglomerativeClustering(distance_threshold=t, kernels=k).fit(X)
    if m.n_clusters_ > 1:
        last = float(np.where(k.live, k.nd, np.inf).min())
    else:
        last = np.inf
    return m.labels_, np.asarray(k.heights, np.float64), last


def oracle_gap(heights, last, t):
    """distance from the threshold to the nearest merge height or to the final nearest distance"""
    v = np.concatenate([np.asarray(heights, np.float64), [last]])
    v = v[np.isfinite(v)]
    return float(np.abs(v - t).min()) if len(v) else np.inf


def blobs(seed, N, D, centres, spread, sub=0, subspread=0.0):
    """unit-free test rows: `centres` Gaussian centres, each optionally split into `sub` sub-centres, plus isotropic noise"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, D))
    if sub:
        c = (c[:, None, :] + subspread * rng.standard_normal((centres, sub, D))).reshape(-1, D)
    return (c[rng.integers(0, len(c), N)] + spread * rng.standard_normal((N, D))).astype(np.float32)
