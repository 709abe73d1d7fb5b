"""TEST-ONLY kernel provider for validate(kernels=...) / topk_acc_device(kernels=...) and the float64 oracle of the GPU tests: the
rules of slic_triplet_val_batch and slic_topk_label_hits (include/slic_hip.h) written out in NumPy float64.  Never shipped, never
imported by the package."""
import numpy as np
import torch


def _np64(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def pair_distance64(x, y, euclid):
    """rowwise 1 - cos with the per-norm clamp 1e-8, or ||x - y + 1e-6||_2, in float64 from the given rows"""
    x, y = _np64(x), _np64(y)
    if euclid:
        return np.sqrt(((x - y + 1e-6) ** 2).sum(1))
    nx = np.maximum(np.sqrt((x * x).sum(1)), 1e-8)
    ny = np.maximum(np.sqrt((y * y).sum(1)), 1e-8)
    return 1.0 - (x * y).sum(1) / (nx * ny)


def val_batch64(ex, ey, ez, euclid, margin):
    """-> (dist_a, dist_b, loss, acc) in float64"""
    da, db = pair_distance64(ex, ey, euclid), pair_distance64(ex, ez, euclid)
    return da, db, np.maximum(da - db + float(margin), 0.0).mean(), float((db - da > 0).sum()) / len(da)


def label_hits(idx, q_labels, g_labels, top_ks):
    """-> (first_hit int32 [Nq], hits int64 [len(top_ks)])"""
    idx = np.asarray(idx)
    q, g = np.asarray(q_labels, dtype=np.int64), np.asarray(g_labels, dtype=np.int64)
    ok = (idx >= 0) & (idx < len(g))
    hit = ok & (g[np.where(ok, idx, 0)] == q[:, None])
    first = np.where(hit.any(1), hit.argmax(1), idx.shape[1]).astype(np.int32)
    return first, np.array([(first < k).sum() for k in top_ks], np.int64)


def topk64(x, y, k, dist_metric):
    x = _np64(x)
    self_search = y is None
    y = x if self_search else _np64(y)
    if dist_metric == 'cosine':
        xn = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
        yn = y / np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-300)
        d = 1.0 - xn @ yn.T
    else:
        d = np.sqrt(np.maximum((x * x).sum(1)[:, None] - 2 * x @ y.T + (y * y).sum(1)[None, :], 0.0))
    if self_search:
        np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)


class NumpyValidationKernels(object):
    def __init__(self):
        self.reads = 0

    def val_batch(self, ex, ey, ez, euclid, margin, rec_row):
        _, _, loss, acc = val_batch64(ex, ey, ez, euclid, margin)
        rec_row[0], rec_row[1], rec_row[2] = float(loss), float(acc), float(ex.shape[0])

    def topk(self, x, y, k, dist_metric):
        return torch.from_numpy(topk64(x, y, k, dist_metric))

    def label_hits(self, idx, q_labels, g_labels, top_ks):
        as_np = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)      # noqa: E731
        return torch.from_numpy(label_hits(as_np(idx), as_np(q_labels), as_np(g_labels), top_ks)[1].astype(np.int32))

    def read_record(self, rec):
        self.reads += 1
        return rec.detach().cpu().numpy()
