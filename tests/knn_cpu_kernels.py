"""TEST-ONLY: the rules of slic_knn_vote and slic_retrieval_ranked (include/slic_hip.h) written out in NumPy, and a provider with
HipKnnKernels' methods for the host logic of neighbors.py / evaluate.knn_classify / retrieval_metrics on a machine without a GPU.

    vote32     the float32 restatement: every operation of the kernel in its order, one rounding each — modes 0 and 1 must agree with
               the device bit for bit (mode 2 takes np.exp in float32, which may differ from the device's expf in the last place)
    vote64     the float64 oracle of the same rules (sequential sums)
    ranked64   the float64 oracle of the ranked metrics and of their means

Never shipped, never imported by the package."""
import numpy as np
import torch

UNIFORM, DISTANCE, SOFTMAX = 0, 1, 2


def _as_np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _votes(idx, g_labels, C):
    """class of every table entry, -1 where it does not vote: padding, gallery label < 0 or >= C"""
    idx, g = np.asarray(idx, dtype=np.int64), np.asarray(g_labels, dtype=np.int64)
    ok = (idx >= 0) & (idx < len(g))
    lab = np.where(ok, g[np.where(ok, idx, 0)], -1)
    return np.where((lab >= 0) & (lab < C), lab, -1)


def _weights(cls, dist, mode, temperature, ft):
    """w [Nq, k] in the float type ft, 0 where the entry does not vote"""
    votes = cls >= 0
    if mode == UNIFORM:
        return np.where(votes, ft(1), ft(0)).astype(ft)
    d = np.asarray(dist).astype(ft)
    w = np.zeros(cls.shape, ft)
    for q in range(cls.shape[0]):
        v = votes[q]
        if not v.any():
            continue
        dq = d[q]
        if mode == DISTANCE:
            if (dq[v] == 0).any():
                w[q] = np.where(v & (dq == 0), ft(1), ft(0))
            else:
                with np.errstate(divide="ignore"):
                    w[q] = np.where(v, ft(1) / np.where(v, dq, ft(1)), ft(0))
        else:
            d_first = dq[np.argmax(v)]
            inv_t = ft(1) / ft(temperature) if ft is np.float32 else 1.0 / float(np.float32(temperature))
            w[q] = np.where(v, np.exp(((d_first - dq) * ft(inv_t)).astype(ft)), ft(0))
    return w


def _rank(s, n_top):
    """the n_top classes by (s descending, class ascending); -1 / 0 past the C-th place"""
    C = s.shape[0]
    order = np.lexsort((np.arange(C), -s.astype(np.float64)))[:n_top]
    pred = np.full(n_top, -1, np.int32)
    score = np.zeros(n_top, s.dtype)
    pred[:len(order)] = order
    score[:len(order)] = s[order]
    return pred, score


def vote32(idx, dist, g_labels, C, mode, temperature, n_top):
    """-> (proba [Nq, C] f32, pred [Nq, n_top] i32, score [Nq, n_top] f32, s [Nq, C] f32: the numerators) as the kernel computes them"""
    cls = _votes(idx, g_labels, C)
    w = _weights(cls, dist, mode, temperature, np.float32)
    Nq, k = cls.shape
    s = np.zeros((Nq, C), np.float32)
    proba = np.zeros((Nq, C), np.float32)
    pred = np.full((Nq, n_top), -1, np.int32)
    score = np.zeros((Nq, n_top), np.float32)
    for q in range(Nq):
        for j in range(k):                                  # rank order, one float32 addition per vote
            if cls[q, j] >= 0:
                s[q, cls[q, j]] = np.float32(s[q, cls[q, j]] + w[q, j])
        if not (cls[q] >= 0).any():
            continue
        lanes = np.zeros(64, np.float32)                    # lane l: s[l], s[l + 64], ... in that order
        for c0 in range(0, C, 64):
            part = s[q, c0:c0 + 64]
            lanes[:len(part)] = lanes[:len(part)] + part
        for o in (32, 16, 8, 4, 2, 1):                      # t += t[lane ^ o]
            lanes = lanes + lanes[np.arange(64) ^ o]
        with np.errstate(divide="ignore", invalid="ignore"):
            proba[q] = s[q] / lanes[0]
        if n_top:
            pred[q], score[q] = _rank(s[q], n_top)
    return proba, pred, score, s


def vote64(idx, dist, g_labels, C, mode, temperature, n_top):
    """the same rules in float64 with sequential sums -> (proba, pred, score, s)"""
    cls = _votes(idx, g_labels, C)
    w = _weights(cls, dist, mode, temperature, np.float64)
    Nq, k = cls.shape
    s = np.zeros((Nq, C), np.float64)
    for q in range(Nq):
        np.add.at(s[q], cls[q][cls[q] >= 0], w[q][cls[q] >= 0])
    tot = s.sum(1, keepdims=True)
    voted = (cls >= 0).any(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        proba = np.where(voted[:, None], s / np.where(tot == 0, 1.0, tot), 0.0)
    pred = np.full((Nq, n_top), -1, np.int32)
    score = np.zeros((Nq, n_top), np.float64)
    for q in range(Nq):
        if voted[q] and n_top:
            pred[q], score[q] = _rank(s[q], n_top)
    return proba, pred, score, s


def ranked64(idx, q_labels, g_labels, n_rel, ks):
    """-> (per_query [Nq, n_ks, 3] = (P, R, AP), rr [Nq], record [3 n_ks + 2]) in float64, one query and one rank at a time"""
    idx = np.asarray(idx, dtype=np.int64)
    q, g, n_rel = np.asarray(q_labels, np.int64), np.asarray(g_labels, np.int64), np.asarray(n_rel, np.int64)
    Nq, k = idx.shape
    per_query = np.zeros((Nq, len(ks), 3), np.float64)
    rr = np.zeros(Nq, np.float64)
    for i in range(Nq):
        hits = [0 <= idx[i, j] < len(g) and g[idx[i, j]] == q[i] for j in range(k)]
        if any(hits):
            rr[i] = 1.0 / (hits.index(True) + 1)
        for a, K in enumerate(ks):
            c, ap = 0, 0.0
            for j in range(K):
                if hits[j]:
                    c += 1
                    ap += c / (j + 1)
            per_query[i, a, 0] = c / K
            if n_rel[i] > 0:
                per_query[i, a, 1] = c / n_rel[i]
                per_query[i, a, 2] = ap / min(n_rel[i], K)
    rel = n_rel > 0
    record = np.zeros(3 * len(ks) + 2, np.float64)
    for a in range(len(ks)):
        record[3 * a] = per_query[:, a, 0].mean()
        if rel.any():
            record[3 * a + 1] = per_query[rel, a, 1].mean()
            record[3 * a + 2] = per_query[rel, a, 2].mean()
    record[3 * len(ks)] = rr.mean()
    record[3 * len(ks) + 1] = rel.sum()
    return per_query, rr, record


def distances64(x, y, dist_metric):
    """[Nq, Ng] float64: 1 - cos of the rows, or the euclidean distance from the differences (equal rows give exactly 0)"""
    x = _as_np(x).astype(np.float64)
    y = x if y is None else _as_np(y).astype(np.float64)
    if dist_metric == 'cosine':
        xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
        yn = y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-300)
        d = np.maximum(1.0 - xn @ yn.T, 0.0)
        d[(xn[:, None, :] == yn[None, :, :]).all(-1)] = 0.0
        return d
    return np.sqrt(((x[:, None, :] - y[None, :, :]) ** 2).sum(-1))


def search64(x, y, k, dist_metric):
    """(idx [Nq, k] int32, dist [Nq, k] float64) ascending, ties to the lower row; y=None: x itself with the diagonal excluded"""
    d = distances64(x, y, dist_metric)
    if y is None:
        np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.take_along_axis(d, idx, axis=1)


class NumpyKnnKernels(object):
    """HipKnnKernels' methods on the host: float64 search (distances handed on as float32, as the device tables hold them), the float32
    restatement of the vote, the float64 ranked metrics.  `calls` records the method names in order."""

    def __init__(self):
        self.reads = 0
        self.calls = []

    def rows(self, x):
        return torch.as_tensor(np.ascontiguousarray(_as_np(x), dtype=np.float32))

    def labels(self, labels):
        return torch.as_tensor(np.ascontiguousarray(_as_np(labels), dtype=np.int64).reshape(-1))

    def search(self, x, y, k, dist_metric, precision="fp32"):
        self.calls.append(("search", int(k), dist_metric))
        idx, d = search64(x, y, k, dist_metric)
        return torch.from_numpy(idx), torch.from_numpy(d.astype(np.float32))

    def vote(self, idx, dist, g_labels, n_classes, mode, temperature, n_top, want_proba):
        self.calls.append(("vote", int(idx.shape[1]), int(mode), int(n_top)))
        proba, pred, score, _ = vote32(_as_np(idx), None if dist is None else _as_np(dist), _as_np(g_labels), n_classes, mode,
                                       temperature, n_top)
        return (torch.from_numpy(proba) if want_proba else None, torch.from_numpy(pred) if n_top else None,
                torch.from_numpy(score) if n_top else None)

    def ranked(self, idx, q_labels, g_labels, n_rel, ks):
        self.calls.append(("ranked", tuple(ks)))
        return tuple(torch.from_numpy(a) for a in ranked64(_as_np(idx), _as_np(q_labels), _as_np(g_labels), _as_np(n_rel), ks))

    def read(self, t):
        self.reads += 1
        return _as_np(t)
