"""
HDBSCAN with the cosine metric on the MI355X: sklearn.cluster.HDBSCAN(min_cluster_size, min_samples, metric='cosine') without a
radius to tune and without sklearn's dense float64 N x N matrix (rules in include/slic_hip.h, slic_hdbscan_core).  The device does the
O(N^2 D) part in csrc/hdbscan.hip: core distances from the library's top-k search, then Boruvka rounds over the mutual-reachability
weights w(i, j) = max(d(i, j), core(i), core(j)): one streamed rows x rows^T pass per round gives every component its lightest edge to
a foreign row, and the N x N matrix is never written.  The host merges the <= C candidate edges of a round through union-find (at most
ceil(log2 N) rounds) and then does what is O(N): the single-linkage tree of the N - 1 edges, the condensed tree, stability, the 'eom' /
'leaf' selection, labels and probabilities, all in plain NumPy / Python from the definition.
Only metric='cosine' is supported.
"""
import ctypes
import time

import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._device import require_device, resident_rows, sized_workspace

HDBSCAN_KMAX = 88              # slic_cosine_topk's list limit: min_samples


# ---------------------------------------------------------------------------------------------------------------------------------
# Boruvka's merge step and the tree order (host, O(N) per round)
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_order(lo, hi, w):
    """the order of rule 4: (w, min(i, j), max(i, j)) ascending"""
    return np.lexsort((hi, lo, w))


def _find(parent, x):
    r = x
    while parent[r] != r:
        r = parent[r]
    while parent[x] != r:
        parent[x], x = r, parent[x]
    return r


def apply_edges(parent, lo, hi, w):
    """unite the candidate edges of one round in the order (w, lo, hi); an edge whose ends are already connected (the same edge found
    from both ends, or a cycle that fp32 scores seen from two ends can close) is dropped.  -> indices of the edges kept, in that order"""
    kept = []
    for e in edge_order(lo, hi, w).tolist():
        a, b = _find(parent, int(lo[e])), _find(parent, int(hi[e]))
        if a == b:
            continue
        if a > b:
            a, b = b, a
        parent[b] = a                                                   # a component's root is its smallest row
        kept.append(e)
    return kept


def components(parent):
    """-> (comp int32 [N] with values 0 .. C-1 numbered by the components' smallest row, C)"""
    p = np.asarray(parent)
    while True:
        q = p[p]
        if np.array_equal(q, p):
            break
        p = q
    roots, comp = np.unique(p, return_inverse=True)
    return comp.astype(np.int32), len(roots)


def boruvka_mst(N, round_fn, weight_fn, stats=None):
    """round_fn(comp int32 [N], C) -> (i, j) int arrays, one candidate edge per component (its two rows in either order; -1 = none);
    weight_fn(pairs [M, 2]) -> float64 w of rule 3.  -> (edges int32 [N-1, 2] with lo < hi, weights float64 [N-1]) in tree order"""
    parent = list(range(N))
    comp, C = np.arange(N, dtype=np.int32), N
    el, eh, ew = [], [], []
    rounds, searched = 0, []
    while C > 1:
        if rounds > 64:
            raise RuntimeError("HDBSCAN: the Boruvka rounds do not converge ({} components left)".format(C))
        i, j = round_fn(comp, C)
        i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
        ok = (i >= 0) & (j >= 0)
        lo, hi = np.minimum(i, j)[ok], np.maximum(i, j)[ok]
        pairs = np.unique(np.stack([lo, hi], axis=1), axis=0)
        if len(pairs) == 0:
            raise RuntimeError("HDBSCAN: a round over {} components proposed no edge".format(C))
        w = np.asarray(weight_fn(pairs.astype(np.int32)), dtype=np.float64)
        kept = apply_edges(parent, pairs[:, 0], pairs[:, 1], w)
        el.append(pairs[kept, 0]); eh.append(pairs[kept, 1]); ew.append(w[kept])
        searched.append(N)
        rounds += 1
        comp, C = components(np.asarray(parent, dtype=np.int64))
    lo, hi, w = np.concatenate(el), np.concatenate(eh), np.concatenate(ew)
    o = edge_order(lo, hi, w)
    if stats is not None:
        stats["rounds"] = rounds
        stats["rows_searched"] = searched
    return np.stack([lo[o], hi[o]], axis=1).astype(np.int32), w[o]


# ---------------------------------------------------------------------------------------------------------------------------------
# from the MST to labels (host, O(N)): the HDBSCAN definition
# ---------------------------------------------------------------------------------------------------------------------------------
def single_linkage(edges, weights, N):
    """edges in tree order -> (left, right, height, size) of the N - 1 merges; merge t makes node N + t"""
    top = list(range(2 * N - 1))                                       # union-find over the nodes, the root is the newest node
    size = [1] * N + [0] * (N - 1)
    left, right = np.empty(N - 1, np.int64), np.empty(N - 1, np.int64)
    for t, (a, b) in enumerate(edges.tolist()):
        ra, rb = _find(top, a), _find(top, b)
        node = N + t
        top[ra] = top[rb] = node
        size[node] = size[ra] + size[rb]
        left[t], right[t] = ra, rb
    return left, right, np.asarray(weights, dtype=np.float64), np.asarray(size[N:], dtype=np.int64)


def _leaves(left, right, N, node):
    out, stack = [], [node]
    while stack:
        n = stack.pop()
        if n < N:
            out.append(n)
        else:
            stack.append(int(left[n - N])); stack.append(int(right[n - N]))
    return out


def condense(left, right, height, size, N, min_cluster_size):
    """the condensed tree.  Clusters are numbered 0 (the root), 1, ... in order of creation (a child after its parent).
    -> cparent, cbirth (lambda at which the cluster splits off), csize per cluster; pparent, plambda per row (the cluster a row falls
    out of and the lambda at which it does)"""
    cparent, cbirth, csize = [-1], [0.0], [N]
    pparent, plambda = np.zeros(N, np.int64), np.zeros(N, np.float64)
    stack = [(2 * N - 2, 0)]
    while stack:
        node, c = stack.pop()
        l, r, h = int(left[node - N]), int(right[node - N]), float(height[node - N])
        lam = 1.0 / h if h > 0.0 else np.inf
        lc = int(size[l - N]) if l >= N else 1
        rc = int(size[r - N]) if r >= N else 1
        for child, cnt, other in ((l, lc, rc), (r, rc, lc)):
            if cnt >= min_cluster_size and other >= min_cluster_size:      # a true split: a new cluster
                cparent.append(c); cbirth.append(lam); csize.append(cnt)
                stack.append((child, len(cparent) - 1))
            elif cnt >= min_cluster_size:                                    # the cluster goes on, the other side falls out
                stack.append((child, c))
            else:
                rows = _leaves(left, right, N, child)
                pparent[rows] = c
                plambda[rows] = lam
    return (np.asarray(cparent, np.int64), np.asarray(cbirth, np.float64), np.asarray(csize, np.int64), pparent, plambda)


def _select(cparent, cbirth, csize, pparent, plambda, method, allow_single_cluster, eps):
    """-> (set of selected clusters, per-cluster death = the largest lambda among the rows and clusters leaving it)"""
    nc = len(cparent)
    with np.errstate(invalid="ignore"):
        stab = np.zeros(nc)
        np.add.at(stab, pparent, plambda - cbirth[pparent])
        np.add.at(stab, cparent[1:], (cbirth[1:] - cbirth[cparent[1:]]) * csize[1:])
    death = np.zeros(nc)
    np.maximum.at(death, pparent, plambda)
    np.maximum.at(death, cparent[1:], cbirth[1:])
    kids = [[] for _ in range(nc)]
    for c in range(1, nc):
        kids[cparent[c]].append(c)

    def below(c):                                                      # the clusters under c, c not included
        out, stack = [], list(kids[c])
        while stack:
            n = stack.pop()
            out.append(n)
            stack.extend(kids[n])
        return out

    def upwards(leaf):
        p = int(cparent[leaf])
        if p == 0:
            return p if allow_single_cluster else leaf
        if 1.0 / cbirth[p] > eps:
            return p
        return upwards(p)

    def epsilon_search(leaves):
        chosen, done = [], set()
        for leaf in sorted(leaves):
            if 1.0 / cbirth[leaf] < eps:
                if leaf not in done:
                    e = upwards(leaf)
                    chosen.append(e)
                    done.update(below(e))
            else:
                chosen.append(leaf)
        return set(chosen)

    nodes = list(range(nc - 1, -1 if allow_single_cluster else 0, -1))
    sel = {c: True for c in nodes}
    if method == 'eom':
        stab = stab.tolist()
        for c in nodes:
            sub = sum(stab[k] for k in kids[c])
            if sub > stab[c]:
                sel[c] = False
                stab[c] = sub
            else:
                for k in below(c):
                    sel[k] = False
        if eps != 0.0 and nc > 1:
            chosen = [c for c in nodes if sel[c]]
            if chosen == [0]:
                picked = set(chosen) if allow_single_cluster else set()
            else:
                picked = epsilon_search(set(chosen))
            sel = {c: c in picked for c in sel}
    else:
        leaves = set(c for c in range(1, nc) if not kids[c])         # no true split at all: nothing is selected
        picked = epsilon_search(leaves) if eps != 0.0 else leaves
        sel = {c: c in picked for c in sel}
    return set(c for c in sel if sel[c]), death


def labels_from_mst(edges, weights, N, min_cluster_size=5, cluster_selection_method='eom', allow_single_cluster=False,
                    cluster_selection_epsilon=0.0):
    """rule 5 and 6 on an MST in tree order -> (labels int32 [N], probabilities float64 [N])"""
    left, right, height, size = single_linkage(np.asarray(edges), weights, N)
    cparent, cbirth, csize, pparent, plambda = condense(left, right, height, size, N, int(min_cluster_size))
    eps = float(cluster_selection_epsilon)
    chosen, death = _select(cparent, cbirth, csize, pparent, plambda, cluster_selection_method, bool(allow_single_cluster), eps)
    # every cluster's nearest selected ancestor (itself included), -1 when the walk reaches the root unselected
    owner = np.full(len(cparent), -1, np.int64)
    for c in range(len(cparent)):                                      # parents come first
        owner[c] = c if c in chosen else (owner[cparent[c]] if c > 0 else -1)
    own = owner[pparent]
    if 0 in chosen and len(chosen) == 1 and allow_single_cluster:
        # the root as the one cluster: a row belongs to it while its own lambda reaches the threshold
        thr = 1.0 / eps if eps != 0.0 else death[0]
        own = np.where((own == 0) & (plambda < thr), -1, own)
    elif 0 in chosen:
        own = np.where(own == 0, -1, own)
    labels = np.full(N, -1, np.int32)
    prob = np.zeros(N, np.float64)
    ok = own >= 0
    if ok.any():
        first = np.full(len(cparent), N, np.int64)
        np.minimum.at(first, own[ok], np.flatnonzero(ok))
        ids = np.flatnonzero(first < N)
        rank = np.full(len(cparent), -1, np.int64)
        rank[ids[np.argsort(first[ids], kind="stable")]] = np.arange(len(ids))      # rule 6: numbered by the smallest row
        labels[ok] = rank[own[ok]]
        dmax = death[own[ok]]
        lam = plambda[ok]
        with np.errstate(invalid="ignore", divide="ignore"):
            prob[ok] = np.where((dmax == 0.0) | np.isinf(lam), 1.0, np.minimum(lam, dmax) / dmax)
    return labels, prob


def cut_labels(edges, weights, N, cut_distance, min_cluster_size=5):
    """sklearn's HDBSCAN.dbscan_clustering: the components of the tree's edges with w < cut_distance, those of fewer than
    min_cluster_size rows are noise; numbered by their smallest row"""
    parent = list(range(N))
    for (a, b), w in zip(np.asarray(edges).tolist(), np.asarray(weights).tolist()):
        if w < cut_distance:
            ra, rb = _find(parent, a), _find(parent, b)
            parent[max(ra, rb)] = min(ra, rb)
    comp, C = components(np.asarray(parent, dtype=np.int64))
    big = np.bincount(comp, minlength=C) >= min_cluster_size
    rank = np.cumsum(big) - 1
    return np.where(big[comp], rank[comp], -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
class HipHdbscanKernels:
    """the device side of HDBSCAN: resident rows, core distances, the MST.  `HDBSCAN(kernels=)` takes another provider with the same
    three methods (tests of the host logic on a GPU-less machine pass a NumPy one as an ARGUMENT; the product has no other)."""

    def __init__(self):
        require_device("HDBSCAN")
        self.last_stats = None
        self._ws = None

    def resident(self, data):
        """fp32 device rows with unit column stride (no copy when they already are)"""
        return resident_rows(data, "HDBSCAN")

    def core_distances(self, rows, min_samples):
        """-> float64 [N] host array (rule 2); leaves the normalised rows and the core distances in the workspace for mst()"""
        N, D = rows.shape
        _lib.require_device(rows)
        self._ws = sized_workspace("slic_hdbscan_workspace_bytes", (N, D, int(min_samples)), rows.device, "hdbscan",
                                   "HDBSCAN: {} x {} rows with min_samples = {} are outside what slic_hdbscan_core takes (2 <= N, 1 <= D "
                                   "<= 512, 1 <= min_samples <= min(N, {}), rows of int32 indices, < 4 GiB padded)"
                                   .format(N, D, min_samples, HDBSCAN_KMAX))
        core = torch.empty(N, dtype=torch.float64, device=rows.device)
        call("slic_hdbscan_core", ptr(rows), N, rows.stride(0), D, int(min_samples), ptr(core), ptr(self._ws), stream())
        self._core = core
        self._ms = int(min_samples)
        self._key = (rows.data_ptr(), N, D)
        return core.cpu().numpy()

    def round(self, rows, comp, C):
        """one Boruvka round -> (lo int32 [C], hi int32 [C], w float32 [C]) host arrays, one candidate per component (-1: none)"""
        N, D = rows.shape
        dev = rows.device
        dcomp = torch.from_numpy(np.ascontiguousarray(comp, dtype=np.int32)).to(dev)
        out = torch.empty(3 * C, dtype=torch.int32, device=dev)
        call("slic_hdbscan_round", ptr(self._ws), N, D, self._ms, ptr(dcomp), int(C), ptr(out[:C]), ptr(out[C:2 * C]), ptr(out[2 * C:]),
             None, stream())
        h = out.cpu().numpy()
        return h[:C].copy(), h[C:2 * C].copy(), h[2 * C:].copy().view(np.float32)

    def edge_weights(self, rows, pairs):
        """float64 w of rule 3 for int32 pairs [M, 2]"""
        N, D = rows.shape
        M = len(pairs)
        if M == 0:
            return np.zeros(0, np.float64)
        dp = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(rows.device)
        out = torch.empty(M, dtype=torch.float64, device=rows.device)
        call("slic_hdbscan_edge_weights", ptr(rows), N, rows.stride(0), D, self._ms, ptr(self._core), ptr(dp), M, ptr(out), ptr(self._ws),
             stream())
        return out.cpu().numpy()

    def mst(self, rows, core=None):
        """-> (edges int32 [N-1, 2], weights float64 [N-1]) in tree order; core_distances(rows, ..) comes first"""
        if self._ws is None or self._key != (rows.data_ptr(),) + tuple(rows.shape):
            raise _lib.SlicError("HDBSCAN: mst() follows core_distances() on the same rows")
        N = rows.shape[0]
        st = {}
        edges, w = boruvka_mst(N, lambda comp, C: self.round(rows, comp, C)[:2], lambda pairs: self.edge_weights(rows, pairs), st)
        dev = (ctypes.c_double * 6)()
        call("slic_hdbscan_stats", dev)
        st.update(ms_core=dev[2], ms_rounds=dev[3], ms_last_round=dev[4], ms_last_pass=dev[5])
        self.last_stats = st
        return edges, w


class HDBSCAN:
    """sklearn-shaped: HDBSCAN(min_cluster_size, min_samples, metric='cosine').fit(X) sets
        labels_          np.int32 [N], -1 = noise; clusters numbered by their smallest row
        probabilities_   np.float64 [N]
        n_clusters_      clusters of labels_ (noise not counted)
        mst_edges_       np.int32 [N-1, 2] (lo, hi), in tree order (w, lo, hi)
        mst_weights_     np.float64 [N-1], the mutual-reachability weights in that order
        core_distances_  np.float64 [N]
        stats_           rounds, rows searched per round, seconds of the device and of the host part
    X: ndarray, CPU tensor, or device tensor (used in place)."""

    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=None, metric='cosine',
                 alpha=1.0, algorithm='auto', cluster_selection_method='eom', allow_single_cluster=False, store_centers=None,
                 kernels=None):
        self.min_cluster_size = min_cluster_size
        self.min_samples = min_samples
        self.cluster_selection_epsilon = cluster_selection_epsilon
        self.max_cluster_size = max_cluster_size
        self.metric = metric
        self.alpha = alpha
        self.algorithm = algorithm
        self.cluster_selection_method = cluster_selection_method
        self.allow_single_cluster = allow_single_cluster
        self.store_centers = store_centers
        self.kernels = kernels

    def fit(self, X, y=None):
        if self.metric != 'cosine':
            raise NotImplementedError("HDBSCAN on the GPU supports metric='cosine' (the metric of the cluster step's embeddings), got "
                                      "{!r}".format(self.metric))
        if self.alpha != 1.0:
            raise NotImplementedError("HDBSCAN on the GPU supports alpha=1.0: the robust-single-linkage scaling of the distances is "
                                      "not built, got {!r}".format(self.alpha))
        if self.max_cluster_size is not None:
            raise NotImplementedError("HDBSCAN on the GPU does not build max_cluster_size (a cap inside the 'eom' selection), got "
                                      "{!r}".format(self.max_cluster_size))
        if self.store_centers is not None:
            raise NotImplementedError("HDBSCAN on the GPU does not build store_centers (centroids / medoids of the clusters), got "
                                      "{!r}".format(self.store_centers))
        if self.algorithm not in ('auto', 'brute'):
            raise NotImplementedError("HDBSCAN on the GPU is an exact all-pairs search (algorithm='auto' or 'brute'): sklearn's trees "
                                      "do not take the cosine metric either, got {!r}".format(self.algorithm))
        if self.cluster_selection_method not in ('eom', 'leaf'):
            raise ValueError("cluster_selection_method must be 'eom' or 'leaf', got {!r}".format(self.cluster_selection_method))
        mcs = self.min_cluster_size
        if int(mcs) != mcs or mcs < 2:
            raise ValueError("min_cluster_size must be an integer >= 2, got {!r}".format(mcs))
        ms = mcs if self.min_samples is None else self.min_samples
        if int(ms) != ms or ms < 1:
            raise ValueError("min_samples must be an integer >= 1, got {!r}".format(ms))
        if not float(self.cluster_selection_epsilon) >= 0.0:
            raise ValueError("cluster_selection_epsilon must be >= 0, got {!r}".format(self.cluster_selection_epsilon))
        mcs, ms = int(mcs), int(ms)
        if not torch.is_tensor(X) and not np.all(np.isfinite(np.asarray(X, dtype=np.float64))):
            raise ValueError("Input X contains NaN or infinity.")
        if torch.is_tensor(X) and not bool(torch.isfinite(X).all()):
            raise ValueError("Input X contains NaN or infinity.")
        k = HipHdbscanKernels() if self.kernels is None else self.kernels     # raises SlicError without a gfx950 device
        rows = k.resident(X)
        N = rows.shape[0]
        if N < 2:
            raise ValueError("n_samples={} while HDBSCAN requires more than one sample".format(N))
        if ms > N:
            raise ValueError("min_samples ({}) must be at most the number of samples in X ({})".format(ms, N))
        if ms > HDBSCAN_KMAX:
            raise NotImplementedError("HDBSCAN on the GPU takes min_samples <= {} (the top-k search's list length), got {}"
                                      .format(HDBSCAN_KMAX, ms))
        t0 = time.perf_counter()
        core = k.core_distances(rows, ms)
        edges, weights = k.mst(rows, core)
        t1 = time.perf_counter()
        labels, prob = labels_from_mst(edges, weights, N, mcs, self.cluster_selection_method, self.allow_single_cluster,
                                       self.cluster_selection_epsilon)
        t2 = time.perf_counter()
        self.core_distances_ = np.asarray(core, dtype=np.float64)
        self.mst_edges_ = np.asarray(edges, dtype=np.int32)
        self.mst_weights_ = np.asarray(weights, dtype=np.float64)
        self.labels_ = labels
        self.probabilities_ = prob
        self.n_clusters_ = int(labels.max()) + 1
        self.stats_ = dict(getattr(k, "last_stats", None) or {})
        self.stats_.update(seconds_mst=t1 - t0, seconds_host_tree=t2 - t1)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def dbscan_clustering(self, cut_distance, min_cluster_size=5):
        """sklearn's method: the flat clustering of a cut of the same tree at cut_distance (DBSCAN* without border rows), on the host
        from the stored MST"""
        return cut_labels(self.mst_edges_, self.mst_weights_, len(self.labels_), float(cut_distance), int(min_cluster_size))
