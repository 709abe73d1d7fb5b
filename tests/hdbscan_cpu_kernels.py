"""TEST-ONLY: the float64 restatement of slic_hdbscan_core's rules (include/slic_hip.h) and a NumPy kernel provider for
HDBSCAN(kernels=...) that mirrors the three device entry points in fp32.  Dense N x N work: N up to a few thousand.  The tree part
(hdbscan_tree_fp64) is written row-list style after the HDBSCAN definition, apart from the product's array form in
clustering/hdbscan.py, so that the two check each other.  Never shipped, never imported by the package."""
import numpy as np

from dbscan_cpu_kernels import inv_norms
from host_rows import host_rows


def distances_fp64(X):
    """rule 1: d = clip(1 - x_i . x_j inv_i inv_j, 0, 2) in float64 from the fp32 rows, d(i, i) = 0, a zero row at 1 from the others"""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    inv = inv_norms(X64)
    d = np.clip(1.0 - (X64 @ X64.T) * inv[:, None] * inv[None, :], 0.0, 2.0)
    d = np.minimum(d, d.T)
    np.fill_diagonal(d, 0.0)
    return d


def core_fp64(d, min_samples):
    """rule 2: the min_samples-th smallest entry of every row, the diagonal zero included"""
    return np.partition(d, min_samples - 1, axis=1)[:, min_samples - 1]


def mutual_reachability(d, core):
    """rule 3"""
    return np.maximum(d, np.maximum(core[:, None], core[None, :]))


class _UF:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, x):
        while self.p[x] != x:
            self.p[x] = self.p[self.p[x]]
            x = self.p[x]
        return x


def kruskal(W):
    """rule 4: the MST of the dense symmetric weights W under the total order (w, min(i, j), max(i, j)).
    -> (edges int32 [N-1, 2], weights [N-1]) in that order"""
    N = len(W)
    lo, hi = np.triu_indices(N, 1)
    w = W[lo, hi]
    order = np.lexsort((hi, lo, w))
    uf = _UF(N)
    E, Wt = [], []
    for e in order.tolist():
        a, b = uf.find(int(lo[e])), uf.find(int(hi[e]))
        if a != b:
            uf.p[max(a, b)] = min(a, b)
            E.append((int(lo[e]), int(hi[e])))
            Wt.append(float(w[e]))
            if len(E) == N - 1:
                break
    return np.asarray(E, dtype=np.int32).reshape(-1, 2), np.asarray(Wt, dtype=W.dtype)


def prim_weights(W):
    """the sorted weights of a minimum spanning tree of W (every MST has the same ones), by Prim's walk in O(N^2)"""
    N = len(W)
    best = W[0].copy()
    done = np.zeros(N, bool)
    done[0] = True
    out = np.empty(N - 1, W.dtype)
    for t in range(N - 1):
        j = int(np.argmin(np.where(done, np.inf, best)))
        out[t] = best[j]
        done[j] = True
        best = np.minimum(best, W[j])
    return np.sort(out)


def hdbscan_tree_fp64(edges, weights, N, min_cluster_size=5, method='eom', allow_single_cluster=False, eps=0.0):
    """rule 5 and 6 on an MST given in the order of rule 4 -> (labels int32 [N], probabilities float64 [N])"""
    # single linkage: node N + t joins the two trees edge t connects
    uf = _UF(2 * N - 1)
    kids, height, count = {}, {}, {i: 1 for i in range(N)}
    for t, ((a, b), w) in enumerate(zip(np.asarray(edges).tolist(), np.asarray(weights).tolist())):
        ra, rb = uf.find(a), uf.find(b)
        uf.p[ra] = uf.p[rb] = N + t
        kids[N + t], height[N + t], count[N + t] = (ra, rb), w, count[ra] + count[rb]

    def points(n):
        out, st = [], [n]
        while st:
            x = st.pop()
            if x < N:
                out.append(x)
            else:
                st.extend(kids[x])
        return out

    # condensed tree as rows (parent cluster, child, lambda, size); clusters are numbered N, N + 1, ... in breadth-first order
    rows, label, nxt = [], {2 * N - 2: N}, N + 1
    level = [2 * N - 2]
    while level:
        below = []
        for n in level:
            l, r = kids[n]
            lam = 1.0 / height[n] if height[n] > 0 else np.inf
            big = [c for c in (l, r) if count[c] >= min_cluster_size]
            for c in (l, r):
                if count[c] < min_cluster_size:
                    rows += [(label[n], p, lam, 1) for p in points(c)]
                elif len(big) == 2:
                    label[c] = nxt
                    nxt += 1
                    rows.append((label[n], c if c < N else label[c], lam, count[c]))
                    below.append(c)
                else:
                    label[c] = label[n]
                    below.append(c)
        level = [c for c in below if c >= N]
    root = N
    crow = {ch: (pa, lam, sz) for pa, ch, lam, sz in rows if sz > 1}          # cluster -> (parent, birth, size)
    birth = {root: 0.0}
    birth.update({c: v[1] for c, v in crow.items()})
    stab = {c: 0.0 for c in birth}
    death = {c: 0.0 for c in birth}
    with np.errstate(invalid="ignore"):
        for pa, ch, lam, sz in rows:
            stab[pa] += (lam - birth[pa]) * sz
            death[pa] = max(death[pa], lam)
    sub = {c: [] for c in birth}
    for c, (pa, _, _) in crow.items():
        sub[pa].append(c)

    def descendants(c):
        out, st = [], list(sub[c])
        while st:
            x = st.pop()
            out.append(x)
            st.extend(sub[x])
        return out

    def up(leaf):
        pa = crow[leaf][0]
        if pa == root:
            return pa if allow_single_cluster else leaf
        return pa if 1.0 / birth[pa] > eps else up(pa)

    def eps_search(cands):
        sel, seen = [], set()
        for c in sorted(cands):
            if 1.0 / birth[c] < eps:
                if c not in seen:
                    e = up(c)
                    sel.append(e)
                    seen.update(descendants(e))
            else:
                sel.append(c)
        return set(sel)

    order = sorted(birth, reverse=True)
    if not allow_single_cluster:
        order = order[:-1]
    chosen = set(order)
    if method == 'eom':
        for c in order:
            s = sum(stab[k] for k in sub[c])
            if s > stab[c]:
                chosen.discard(c)
                stab[c] = s
            else:
                chosen -= set(descendants(c))
        if eps != 0.0 and crow:
            if chosen == {root}:
                chosen = chosen if allow_single_cluster else set()
            else:
                chosen = eps_search(chosen) & set(order)
    else:
        leaves = set(c for c in crow if not sub[c])
        chosen = (eps_search(leaves) if eps != 0.0 else leaves) & set(order)

    labels = np.full(N, -1, np.int64)
    prob = np.zeros(N)
    single = chosen == {root} and allow_single_cluster
    thr = (1.0 / eps if eps != 0.0 else death[root]) if single else None
    for pa, ch, lam, sz in rows:
        if sz > 1:
            continue
        c = pa
        while c not in chosen and c != root:
            c = crow[c][0]
        if c not in chosen or (c == root and not (single and lam >= thr)):
            continue
        labels[ch] = c
        prob[ch] = 1.0 if death[c] == 0.0 or np.isinf(lam) else min(lam, death[c]) / death[c]
    return renumber(labels), prob


def renumber(labels):
    """rule 6: clusters numbered 0, 1, ... by their smallest row, noise stays -1"""
    labels = np.asarray(labels)
    out = np.full(len(labels), -1, np.int32)
    nxt = 0
    seen = {}
    for i, l in enumerate(labels.tolist()):
        if l >= 0:
            if l not in seen:
                seen[l] = nxt
                nxt += 1
            out[i] = seen[l]
    return out


def cut_fp64(edges, weights, N, cut, min_cluster_size):
    """dbscan_clustering: components of the tree edges with w < cut, small ones are noise"""
    uf = _UF(N)
    for (a, b), w in zip(np.asarray(edges).tolist(), np.asarray(weights).tolist()):
        if w < cut:
            ra, rb = uf.find(a), uf.find(b)
            uf.p[max(ra, rb)] = min(ra, rb)
    root = np.asarray([uf.find(i) for i in range(N)])
    size = np.bincount(root, minlength=N)
    return renumber(np.where(size[root] >= min_cluster_size, root, -1))


def hdbscan_fp64(X, min_cluster_size=5, min_samples=None, method='eom', allow_single_cluster=False, eps=0.0):
    """-> dict(labels, probabilities, edges, weights, core) by rules 1-6 in float64"""
    d = distances_fp64(X)
    ms = min_cluster_size if min_samples is None else min_samples
    core = core_fp64(d, ms)
    edges, weights = kruskal(mutual_reachability(d, core))
    labels, prob = hdbscan_tree_fp64(edges, weights, len(d), min_cluster_size, method, allow_single_cluster, eps)
    return dict(labels=labels, probabilities=prob, edges=edges, weights=weights, core=core)


def same_partition(a, b):
    """two labelings describe one partition (noise = -1 matches noise)"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


def is_spanning_tree(edges, N):
    """N - 1 edges, acyclic and connected"""
    edges = np.asarray(edges)
    if edges.shape != (N - 1, 2):
        return False
    uf = _UF(N)
    for a, b in edges.tolist():
        ra, rb = uf.find(a), uf.find(b)
        if ra == rb:
            return False
        uf.p[ra] = rb
    return True


class NumpyHdbscanKernels:
    """the HipHdbscanKernels interface on host arrays, with the device's arithmetic: fp32 unit rows and fp32 scores for the search,
    float64 for the values that are reported.  defect: one deliberate error, for the tests that must catch it."""

    def __init__(self, defect=None):
        self.defect = defect
        self.last_stats = None

    def resident(self, data):
        return host_rows(data, "HDBSCAN")

    def _prepare(self, rows):
        X64 = rows.astype(np.float64)
        self.Xn = (X64 * inv_norms(X64)[:, None]).astype(np.float32)
        S = self.Xn @ self.Xn.T
        S = np.triu(S) + np.triu(S, 1).T                                # one fp32 score per pair
        self.d32 = np.clip(np.float32(1.0) - S, np.float32(0.0), np.float32(2.0)).astype(np.float32)
        self.d64 = distances_fp64(rows)

    def core_distances(self, rows, min_samples):
        """slic_hdbscan_core: the min_samples-th entry of the fp32 list (ties -> lower row, the row itself in it), rescored in float64"""
        self._prepare(rows)
        N = len(rows)
        d = self.d32.copy()
        k = min_samples
        if self.defect == 'no_diagonal':
            np.fill_diagonal(d, np.inf)                                 # the error: the row itself is not counted
        jk = np.argsort(d, axis=1, kind="stable")[:, min(k, N) - 1]
        if k == 1 and self.defect != 'no_diagonal':
            jk = np.arange(N)                                           # the diagonal zero itself (a zero row scores 0 against itself)
        self.core = self.d64[np.arange(N), jk]
        self.core32 = self.core.astype(np.float32)
        return self.core.copy()

    def weights32(self):
        return np.maximum(self.d32, np.maximum(self.core32[:, None], self.core32[None, :]))

    def round(self, rows, comp, C):
        """slic_hdbscan_round: every row's lightest foreign row (ties -> lower row), then the least (w, lo, hi) of every component"""
        W = self.weights32().astype(np.float64)
        N = len(W)
        if self.defect != 'no_mask':
            W[comp[:, None] == comp[None, :]] = np.inf
        if self.defect == 'larger_j':
            j = N - 1 - np.argmin(W[:, ::-1], axis=1)
        else:
            j = np.argmin(W, axis=1)
        w = W[np.arange(N), j]
        i = np.arange(N)
        lo, hi = np.minimum(i, j), np.maximum(i, j)
        oi, oj, ow = np.full(C, -1, np.int32), np.full(C, -1, np.int32), np.full(C, np.inf, np.float32)
        for r in np.lexsort((hi, lo, w))[::-1].tolist():                # the least key is written last
            if np.isfinite(w[r]):
                oi[comp[r]], oj[comp[r]], ow[comp[r]] = lo[r], hi[r], w[r]
        return oi, oj, ow

    def edge_weights(self, rows, pairs):
        """slic_hdbscan_edge_weights"""
        a, b = pairs[:, 0], pairs[:, 1]
        return np.maximum(self.d64[a, b], np.maximum(self.core[a], self.core[b]))

    def mst(self, rows, core=None):
        from video_similarity_search_amd.clustering.hdbscan import boruvka_mst
        st = {}
        if self.defect == 'keep_cycles':
            return self._mst_keeping_cycles(rows)
        out = boruvka_mst(len(rows), lambda comp, C: self.round(rows, comp, C)[:2], lambda p: self.edge_weights(rows, p), st)
        self.last_stats = st
        return out

    def _mst_keeping_cycles(self, rows):
        """the error: the candidate edges of a round are all kept, also the one that closes a cycle"""
        from video_similarity_search_amd.clustering.hdbscan import components, edge_order
        N = len(rows)
        parent = np.arange(N)
        comp, C = np.arange(N, dtype=np.int32), N
        E = []
        while C > 1:
            i, j, _ = self.round(rows, comp, C)
            for a, b in zip(i.tolist(), j.tolist()):                    # (lo, hi) of both ends: not even de-duplicated
                E.append((a, b))
                uf = _UF(N)
                uf.p = parent.tolist()
                ra, rb = uf.find(a), uf.find(b)
                parent[max(ra, rb)] = min(ra, rb)
            comp, C = components(parent)
        E = np.asarray(E, dtype=np.int32)
        w = self.edge_weights(rows, E)
        o = edge_order(E[:, 0], E[:, 1], w)
        return E[o], w[o]
