"""The float64 oracle of slic_pair_stats (include/slic_hip.h) and a NumPy provider for the host logic of pairstats.py.

pair_stats_fp64 follows the header's rules with every distance in float64: inv = 1 / ||x|| (0 for a zero row), d = clip(1 - (x_i . x_j)
inv_i inv_j, 0, 2), bin = min(bins - 1, floor(d bins / 2)), group 1 iff both rows are labelled alike, ignored rows in no pair, the self
form over i < j.  It keeps the sorted distances of either group, so a test can count the pairs below any threshold."""
import numpy as np

U = 2.0 ** -24
RECORD = 9


def delta(D):
    """the bound on |d_device - d_float64| for unit rows rounded to fp32 and a length-D fp32 product chain (the silhouette's bound for
    the same operand form): (D + 8) 2^-24"""
    return (D + 8) * U


def pair_stats_fp64(x, x_labels=None, y=None, y_labels=None, bins=256, t=2.0, ignore_label=None):
    """-> {'hist': int64 [2, bins] (row 0 diff, row 1 same), 'record': float64 [9], 'd': (sorted diff distances, sorted same distances)}"""
    x64 = np.asarray(x, dtype=np.float64)
    self_form = y is None
    y64 = x64 if self_form else np.asarray(y, dtype=np.float64)
    lx = None if x_labels is None else np.asarray(x_labels).astype(np.int64)
    ly = lx if self_form else (None if y_labels is None else np.asarray(y_labels).astype(np.int64))

    def inv(a):
        n = np.sqrt((a * a).sum(axis=1))
        return np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)

    d = np.clip(1.0 - (x64 @ y64.T) * inv(x64)[:, None] * inv(y64)[None, :], 0.0, 2.0)
    valid = np.ones(d.shape, dtype=bool)
    if self_form:
        valid &= np.triu(np.ones(d.shape, dtype=bool), 1)
    if ignore_label is not None:
        if lx is not None:
            valid &= (lx != ignore_label)[:, None]
        if ly is not None:
            valid &= (ly != ignore_label)[None, :]
    same = (lx[:, None] == ly[None, :]) if lx is not None and ly is not None else np.zeros(d.shape, dtype=bool)
    tt = float(np.float32(2.0 * t))
    hist = np.zeros((2, bins), dtype=np.int64)
    rec = np.zeros(RECORD)
    ds = []
    for g in (0, 1):
        dg = np.sort(d[valid & (same == bool(g))])
        ds.append(dg)
        b = np.minimum(bins - 1, np.floor(dg * (bins / 2)).astype(np.int64))
        hist[g] = np.bincount(b, minlength=bins)
        rec[g] = dg.size
        rec[2 + g] = dg.sum()
        rec[4 + g] = (dg * dg).sum()
        rec[6 + g] = np.exp(-tt * dg).sum()
    return {"hist": hist, "record": rec, "d": tuple(ds)}


class NumpyPairStatsKernels:
    """the provider pairstats.py's functions take through `kernels=`: the oracle behind HipPairStatsKernels' three methods; `calls`
    lists what was asked"""

    def __init__(self):
        self.calls = []

    def resident_rows(self, X):
        a = X.detach().cpu().numpy() if hasattr(X, "detach") else np.asarray(X)
        if a.ndim != 2:
            raise ValueError("2-D rows expected")
        return np.ascontiguousarray(a, dtype=np.float32)

    def resident_labels(self, labels):
        a = labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels)
        return np.ascontiguousarray(a, dtype=np.int32)

    def pair_stats(self, x, x_labels, y, y_labels, bins, t, ignore_label=None):
        self.calls.append(("pair_stats", x.shape, None if y is None else y.shape, x_labels is not None, y_labels is not None, bins, t,
                           ignore_label))
        o = pair_stats_fp64(x, x_labels, y, y_labels, bins, t, ignore_label)
        return o["hist"], o["record"]
