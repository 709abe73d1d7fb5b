"""TEST-ONLY kernel provider for OPTICS(kernels=...) and the float64 oracle of the GPU tests: the rules of slic_optics_cosine
(include/slic_hip.h) written out directly in NumPy on the full N x N float64 distance matrix (N up to a few thousand).  The walk (rules
1-4) and the closed-form labels (rule 5) are computed separately, so that one can check the other.  Never shipped, never imported by the
package."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from host_rows import host_rows


def fp64_distances(X):
    """rule 1's distance: float64 from the raw fp32 rows, d(i, i) = 0, a zero row at distance 1 from every other row"""
    X = np.asarray(X, dtype=np.float64)
    n = np.sqrt(np.einsum("ij,ij->i", X, X))
    inv = np.zeros_like(n)
    np.divide(1.0, n, out=inv, where=n > 0)
    d = np.clip(1.0 - ((X @ X.T) * inv[:, None]) * inv[None, :], 0.0, 2.0)
    np.fill_diagonal(d, 0.0)
    return d


def core_distances(d, max_eps, min_samples):
    """-> (is_core, core_dist): rules 2 and 3 on a distance matrix"""
    core = (d <= max_eps).sum(axis=1) >= min_samples
    kth = np.partition(d, min_samples - 1, axis=1)[:, min_samples - 1]        # the row's own 0 is the first of them
    return core, np.where(core, kth, np.inf)


def walk(d, core, cd, max_eps, want_gap=False):
    """rule 4 -> (ordering, reachability, predecessor[, gap]).  gap = the smallest margin any pick or relax comparison had:
    second-smallest minus smallest DISTINCT finite reachability at a pick, |r - reachability[j]| at a relax where the two differ."""
    N = len(d)
    reach = np.full(N, np.inf)
    pred = np.full(N, -1, np.int64)
    done = np.zeros(N, bool)
    order = np.empty(N, np.int64)
    gap = np.inf
    for t in range(N):
        cand = np.flatnonzero(~done)
        r = reach[cand]
        p = cand[np.argmin(r)]                     # argmin takes the first of equal values: the lowest row index
        if want_gap:
            f = np.unique(r[np.isfinite(r)])
            if len(f) > 1:
                gap = min(gap, f[1] - f[0])
        done[p] = True
        order[t] = p
        if core[p]:
            nb = np.flatnonzero(~done & (d[p] <= max_eps))
            rn = np.maximum(d[p, nb], cd[p])
            if want_gap:
                fin = np.isfinite(reach[nb]) & (rn != reach[nb])
                if fin.any():
                    gap = min(gap, np.abs(rn[fin] - reach[nb][fin]).min())
            upd = rn < reach[nb]
            reach[nb[upd]] = rn[upd]
            pred[nb[upd]] = p
    return (order, reach, pred, gap) if want_gap else (order, reach, pred)


def closed_form_labels(d, core, max_eps):
    """rule 5 -> (labels, n_clusters), without the walk"""
    N = len(d)
    labels = np.full(N, -1, np.int64)
    cidx = np.flatnonzero(core)
    if not len(cidx):
        return labels, 0
    a, b = np.nonzero(d[np.ix_(cidx, cidx)] <= max_eps)
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(len(cidx), len(cidx)))
    ncl, comp = connected_components(g, directed=False)
    first = np.full(ncl, N, np.int64)                                         # smallest core row of every component
    np.minimum.at(first, comp, cidx)
    rank = np.empty(ncl, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(ncl)
    labels[cidx] = rank[comp]
    start = np.sort(first)                                                    # start[c] = smallest core row of cluster c
    for b_ in np.flatnonzero(~core):
        nb = cidx[d[b_, cidx] <= max_eps]
        if len(nb):
            c = labels[nb].min()                                              # smallest number = smallest start row
            labels[b_] = c if start[c] < b_ else -1
    return labels, int(ncl)


def optics_fp64(X, max_eps, min_samples, want_gap=False):
    """-> dict(labels, is_core, core_distances, ordering, reachability, predecessor, n_clusters[, gap]) by rules 1-5 in float64.
    gap (want_gap): the smallest of the distance of any pair from max_eps, the spacing of every row's first min_samples + 1 sorted
    distances, and the walk's own margins (see walk)."""
    X = np.asarray(X, dtype=np.float32)
    d = fp64_distances(X)
    core, cd = core_distances(d, max_eps, min_samples)
    labels, ncl = closed_form_labels(d, core, max_eps)
    out = dict(labels=labels.astype(np.int32), is_core=core, core_distances=cd, n_clusters=ncl)
    if want_gap:
        order, reach, pred, gap = walk(d, core, cd, max_eps, True)
        off = ~np.eye(len(X), dtype=bool)
        gap = min(gap, np.abs(d[off] - max_eps).min())
        first = np.sort(d, axis=1)[:, :min_samples + 1]
        gap = min(gap, np.diff(first, axis=1).min())
        out["gap"] = float(gap)
    else:
        order, reach, pred = walk(d, core, cd, max_eps)
    out.update(ordering=order.astype(np.int32), reachability=reach, predecessor=pred.astype(np.int32))
    return out


class NumpyOpticsKernels:
    """the HipOpticsKernels interface on host arrays"""

    def __init__(self):
        self.last_stats = None

    def resident(self, data):
        return host_rows(data, "OPTICS")

    def optics(self, rows, max_eps, min_samples, walk=True):
        o = optics_fp64(rows, max_eps, min_samples)
        if not walk:
            return o["labels"], o["is_core"], None, None, None, None, o["n_clusters"]
        return (o["labels"], o["is_core"], o["core_distances"].astype(np.float32), o["reachability"].astype(np.float32),
                o["predecessor"], o["ordering"], o["n_clusters"])
