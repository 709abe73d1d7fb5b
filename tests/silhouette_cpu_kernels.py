"""NumPy stand-ins for the silhouette call (csrc/silhouette.hip), for tests on a machine without a GPU:

  silhouette_fp64     the plain definition in float64 from the N x N distance matrix (what sklearn computes): the reference of
                      every gate.  It shares nothing with the cluster-sum identity the kernel rests on.
  silhouette_mirror   the kernel's arithmetic in its rounding order: float64 statistics rounded once to fp32, a k-ascending fp32
                      fmaf chain for the dot products, the fp32 epilogue.  An fmaf is restated as a float64 multiply-add rounded to
                      fp32; that is a double rounding, so a value may differ from the device's in its last bit — the mirror is held
                      to the same derived gate as the device, not to bit equality.  `defect` injects one of DEFECTS.
  NumpySilhouetteKernels   the provider the host driver (clustering/metrics.py) takes through `kernels=`: the mirror behind the
                      methods of HipSilhouetteKernels, with the call's status rules.
  gates               the derived per-row gate of the issue: 4 delta / max(a64, b64), rows with max(a64, b64) < 0.05 left out.
"""
import numpy as np

from host_rows import host_labels, host_rows

DEFECTS = ("self_kept", "n_for_n_minus_1", "own_in_b", "singleton_kept", "ties_last")
U = 2.0 ** -24
F32, F64 = np.float32, np.float64


def _groups(labels, ignore_label):
    """dense ids by ascending label value (-1 for ignored rows), the label values, the counts"""
    labels = np.asarray(labels)
    keep = np.ones(len(labels), bool) if ignore_label is None else labels != ignore_label
    vals, inv = np.unique(labels[keep], return_inverse=True)
    ids = np.full(len(labels), -1, np.int64)
    ids[keep] = inv
    return ids, vals, np.bincount(inv, minlength=len(vals))


def _unit_rows64(x):
    n = np.sqrt((x * x).sum(1))
    return np.divide(x, n[:, None], out=np.zeros_like(x), where=n[:, None] > 0)


def silhouette_fp64(X, labels, metric="cosine", ignore_label=None):
    """-> dict(s, a, b, nearest, score, cluster_label, cluster_mean, n_clusters, n_rows), float64; NaN rows for ignored labels"""
    x = np.asarray(X, F64)
    ids, vals, cnt = _groups(labels, ignore_label)
    keep = ids >= 0
    xs, idk = x[keep], ids[keep]
    if metric == "cosine":
        xh = _unit_rows64(xs)
        dist = 1.0 - xh @ xh.T
    else:
        n2 = (xs * xs).sum(1)
        dist = np.maximum(n2[:, None] + n2[None, :] - 2.0 * (xs @ xs.T), 0.0)
    np.fill_diagonal(dist, 0.0)
    K, n = len(vals), len(idk)
    onehot = np.zeros((n, K))
    onehot[np.arange(n), idk] = 1.0
    tot = dist @ onehot                                       # [n, K] sum of distances to every cluster
    own_n = cnt[idk]
    a = np.where(own_n > 1, tot[np.arange(n), idk] / np.maximum(own_n - 1, 1), 0.0)
    mean = tot / cnt[None, :]
    mean[np.arange(n), idk] = np.inf
    near = mean.argmin(1)                                     # the first index among equals
    b = mean[np.arange(n), near]
    m = np.maximum(a, b)
    s = np.where((own_n > 1) & (m > 0), (b - a) / np.where(m > 0, m, 1.0), 0.0)
    def full(v, fill):
        o = np.full(len(ids), fill, np.asarray(v).dtype)
        o[keep] = v
        return o

    cm = np.array([s[idk == c].mean() for c in range(K)])
    return dict(s=full(s, np.nan), a=full(a, np.nan), b=full(b, np.nan),
                nearest=full(vals[near].astype(np.int64), 0 if ignore_label is None else ignore_label), ids=ids,
                score=float(s.mean()), cluster_label=vals, cluster_mean=cm, n_clusters=K, n_rows=n)


def _fmaf(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def silhouette_mirror(X, labels, metric="cosine", ignore_label=None, defect=None):
    """the kernel's rounding order; same keys as silhouette_fp64, s / a / b in fp32, means in float64"""
    assert defect is None or defect in DEFECTS
    x = np.asarray(X, F32)
    N, D = x.shape
    cosine = metric == "cosine"
    ids, vals, cnt = _groups(labels, ignore_label)
    K = len(vals)
    # prep: |x|^2 in float64, k ascending; the operand row in fp32; the self term as the fmaf chain gives it
    n2 = np.zeros(N)
    for k in range(D):
        n2 += x[:, k].astype(F64) * x[:, k].astype(F64)
    if cosine:
        nrm = np.sqrt(n2)
        op = np.divide(x.astype(F64), nrm[:, None], out=np.zeros((N, D)), where=nrm[:, None] > 0).astype(F32)
    else:
        op = x
    dot_self = np.zeros(N, F32)
    for k in range(D):
        dot_self = _fmaf(op[:, k], op[:, k], dot_self)
    self_t = (F32(1.0) - dot_self) if cosine else np.zeros(N, F32)
    xn = np.zeros(N, F32) if cosine else n2.astype(F32)
    # stats: float64 sums in ascending row order, one rounding to fp32
    mean = np.zeros((K, D), F32)
    q = np.ones(K, F32)
    for c in range(K):
        rows = np.flatnonzero(ids == c)
        mean[c] = (np.cumsum(op[rows].astype(F64), axis=0)[-1] / float(len(rows))).astype(F32)
        if not cosine:
            q[c] = F32(np.cumsum(n2[rows])[-1] / float(len(rows)))
    # score: k-ascending fmaf chain from +0, then max(fmaf(-alpha, dot, xn + q), 0)
    dot = np.zeros((N, K), F32)
    for k in range(D):
        dot = _fmaf(op[:, k][:, None], mean[:, k][None, :], dot)
    alpha = F32(-1.0 if cosine else -2.0)
    d = np.maximum(_fmaf(alpha, dot, (xn[:, None] + q[None, :]).astype(F32)), F32(0.0))
    keep = ids >= 0
    r = np.arange(N)
    idc = np.where(keep, ids, 0)
    own = d[r, idc]
    other = d.copy()
    if defect != "own_in_b":
        other[r, idc] = np.inf
    near = (K - 1 - other[:, ::-1].argmin(1)) if defect == "ties_last" else other.argmin(1)
    b = other[r, near]
    n_own = cnt[idc].astype(F32)
    tot = _fmaf(n_own, own, np.zeros(N, F32) if defect == "self_kept" else -self_t)
    tot = np.maximum(tot, F32(0.0))
    den = n_own if defect == "n_for_n_minus_1" else n_own - F32(1.0)
    single = cnt[idc] <= 1
    a = np.where(single, F32(0.0), tot / np.where(den > 0, den, F32(1.0))).astype(F32)
    m = np.maximum(a, b)
    s = np.where(m == 0, F32(0.0), (b - a) / np.where(m == 0, F32(1.0), m)).astype(F32)
    if defect == "singleton_kept":
        s = np.where(single, np.where(b > 0, F32(1.0), F32(0.0)), s).astype(F32)      # (b - 0) / b: what a missing rule leaves
    else:
        s = np.where(single, F32(0.0), s).astype(F32)
    nan = F32(np.nan)
    s, a, b = (np.where(keep, v, nan).astype(F32) for v in (s, a, b))
    nearest = np.where(keep, vals[near] if K else 0, 0 if ignore_label is None else ignore_label).astype(np.int32)
    s64 = s[keep].astype(F64)
    cm = np.array([s[ids == c].astype(F64).mean() for c in range(K)])
    return dict(s=s, a=a, b=b, nearest=nearest, score=float(s64.mean()) if keep.any() else float("nan"),
                cluster_label=vals.astype(np.int32), cluster_mean=cm, n_clusters=K, n_rows=int(keep.sum()))


def deltas(X, ref, metric):
    """the derived bound [N] on the error of one mean distance: (D + 8) u for cosine, (D + 8) u (|x_i| + R)^2 with
    R^2 = max_C Q_C / |C| for sqeuclidean (a: at most 2 delta, b: at most delta)"""
    x = np.asarray(X, F64)
    D = x.shape[1]
    if metric == "cosine":
        return np.full(len(x), (D + 8) * U)
    n2 = (x * x).sum(1)
    R2 = max(n2[ref["ids"] == c].mean() for c in range(ref["n_clusters"]))
    return (D + 8) * U * (np.sqrt(n2) + np.sqrt(R2)) ** 2


def gates(X, ref, metric):
    """(gate [N], gated [N] bool) from the float64 reference `ref` = silhouette_fp64(...): 4 delta_i / max(a64, b64); rows with
    max(a64, b64) < 0.05 (and ignored rows) are left out"""
    m = np.maximum(ref["a"], ref["b"])
    with np.errstate(invalid="ignore", divide="ignore"):
        gate = 4.0 * deltas(X, ref, metric) / m
    gated = ~np.isnan(ref["s"]) & (m >= 0.05)
    return gate, gated


def check_rows(got_s, X, ref, metric, what=""):
    """the issue's gate: every gated row within its gate, at most 1 % of the scored rows left out; prints and returns
    (worst error, its slack = gate / error, rows left out)"""
    gate, gated = gates(X, ref, metric)
    scored = ~np.isnan(ref["s"])
    left_out = int(scored.sum() - gated.sum())
    err = np.abs(np.asarray(got_s, F64) - ref["s"])
    worst = int(np.argmax(np.where(gated, err / gate, -1.0)))
    print("{}: worst |s - s64| = {:.3e} (gate {:.3e}, slack x{:.1f}), rows left out of the gate {} / {}".format(
        what, err[worst], gate[worst], gate[worst] / max(err[worst], 1e-300), left_out, int(scored.sum())))
    assert left_out <= 0.01 * scored.sum(), (what, left_out)
    assert np.array_equal(np.isnan(np.asarray(got_s)), ~scored), what
    bad = np.flatnonzero(gated & ~(err <= gate))
    assert bad.size == 0, (what, bad[:5], err[bad[:5]], gate[bad[:5]])
    return float(err[worst]), float(gate[worst] / max(err[worst], 1e-300)), left_out


def check_mean(got, X, ref, metric, what=""):
    """the mean is gated at the mean of the row gates (over the gated rows)"""
    gate, gated = gates(X, ref, metric)
    g = float(gate[gated].mean())
    print("{}: |score - score64| = {:.3e} (gate {:.3e})".format(what, abs(got - ref["score"]), g))
    assert abs(got - ref["score"]) <= g, (what, got, ref["score"], g)


class NumpySilhouetteKernels:
    """HipSilhouetteKernels' methods on host arrays, the mirror underneath; status rules as slic_silhouette's"""

    def __init__(self, max_clusters=None, defect=None):
        self.max_clusters, self.defect = max_clusters, defect

    def resident_rows(self, X):
        assert not (hasattr(X, "is_cuda") and X.is_cuda)
        return host_rows(X, "the silhouette")

    resident_labels = staticmethod(host_labels)

    def take(self, x, idx):
        return x[np.asarray(idx, np.int64)]

    def n_labels(self, labels):
        return len(np.unique(labels))

    def silhouette(self, X, labels, metric, ignore_label=None, rows=True, clusters=True):
        N = X.shape[0]
        kmax = N - 1 if self.max_clusters is None else min(self.max_clusters, N - 1)
        name = {0: "cosine", 1: "sqeuclidean"}[metric]
        ids, vals, cnt = _groups(labels, ignore_label)
        K, n = len(vals), int((ids >= 0).sum())
        status = 1 if (K < 2 or K > n - 1) else 2 if K > kmax else 0
        out = {"max_clusters": kmax}
        if status:
            out["record"] = np.array([np.nan, K, n, status])
            return out
        m = silhouette_mirror(X, labels, name, ignore_label, self.defect)
        out["record"] = np.array([m["score"], K, n, 0.0])
        if rows:
            out.update(s=m["s"], a=m["a"], b=m["b"], nearest=m["nearest"])
        if clusters:
            out.update(cluster_mean=m["cluster_mean"], cluster_label=m["cluster_label"])
        return out
