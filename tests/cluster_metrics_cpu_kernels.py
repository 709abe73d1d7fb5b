"""A NumPy float64 provider for clustering/metrics.py with the methods of HipClusterMetricsKernels: the rules of
include/slic_hip.h (slic_cluster_metrics) restated on the host IN THE KERNEL'S SUMMATION ORDER, so that the device and this file
differ only in the last bits of lgamma / log / exp.  Test infrastructure: passed as `kernels=`; the product has no CPU path."""
import math

import numpy as np

from host_rows import host_labels

G, T = 1024, 256                     # CM_G workgroups x CM_T threads of every fixed-order sum
MAX_CELLS = 1 << 26                  # SLIC_METRICS_MAX_CELLS
EPS = float(np.finfo(np.float64).eps)

try:
    from scipy.special import gammaln as _gammaln
except ImportError:                                                                                   # pragma: no cover
    _gammaln = np.vectorize(math.lgamma, otypes=[np.float64])


def _fold(v):
    """[..., 256] -> [...]: v[t] += v[t + s] for s = 128 .. 1, as one workgroup does it"""
    v = np.array(v, dtype=np.float64)
    o = v.shape[-1] // 2
    while o > 0:
        v[..., :o] += v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def grid_partials(terms):
    """the 1024 partial sums of a 1-D array of per-cell terms: cell p belongs to thread p mod (1024 * 256), a thread adds its
    cells in ascending p, a workgroup folds its 256 threads by halving"""
    S = G * T
    terms = np.asarray(terms, dtype=np.float64)
    acc = np.zeros(S)
    for s in range(0, len(terms), S):
        row = terms[s:s + S]
        acc[:len(row)] += row
    return _fold(acc.reshape(G, T))


def final_sum(partials):
    """one workgroup over the 1024 partials: thread t adds t, t + 256, t + 512, t + 768 in this order, then the same halving"""
    p = np.asarray(partials, dtype=np.float64).reshape(4, T)
    return float(_fold(((p[0] + p[1]) + p[2]) + p[3]))


def grid_sum(terms):
    return final_sum(grid_partials(terms))


def scan_f64(v):
    """exclusive scan in the order of cm_scan_f64: 1024 runs of ceil(n / 1024) consecutive elements, each summed in ascending
    order from 0; the run sums scanned by doubling; each run re-added in ascending order onto the sum of the runs before it"""
    n, W = len(v), 1024
    per = -(-n // W)
    runs = np.zeros((W, per))
    runs.reshape(-1)[:n] = v
    s = np.cumsum(np.concatenate([np.zeros((W, 1)), runs], axis=1), axis=1)[:, -1]
    o = 1
    while o < W:
        s = np.concatenate([s[:o], s[o:] + s[:-o]])
        o *= 2
    base = np.concatenate([[0.0], s[:-1]])
    out = np.cumsum(np.concatenate([base[:, None], runs], axis=1), axis=1)[:, :-1]
    return out.reshape(-1)[:n]


def t_table(N):
    """T(x) = sum_{k < x} log1p(-k / N), x = 0 .. N"""
    t = np.zeros(N + 1)
    t[:N] = np.log1p(-(np.arange(N, dtype=np.float64) / float(N)))
    return scan_f64(t)


def emi_cells(a, b, N, lg, ln, tl):
    """per (class, cluster) cell, row-major: sum over n = max(1, a + b - N) .. min(a, b), ascending, of the EMI term"""
    R, C = len(a), len(b)
    ai = np.repeat(a.astype(np.int64), C)
    bj = np.tile(b.astype(np.int64), R)
    lo = np.maximum(1, ai + bj - N)
    hi = np.minimum(ai, bj)
    pre = lg[ai] + lg[bj]
    la, lb, ta, tb = ln[ai], ln[bj], tl[ai], tl[bj]
    lnN, dN = ln[N], float(N)
    cell = np.zeros(R * C)
    n = lo.copy()
    act = np.flatnonzero(n <= hi)
    while act.size:
        m, x, y = n[act], ai[act], bj[act]
        term1 = m / dN
        term2 = ((lnN + ln[m]) - la[act]) - lb[act]
        g = ((((pre[act] - lg[m]) - lg[x - m]) - lg[y - m]) - m * lnN) + ((tl[x + y - m] - ta[act]) - tb[act])
        cell[act] += (term1 * term2) * np.exp(g)
        n[act] += 1
        act = act[n[act] <= hi[act]]
    return cell


def cluster_metrics_fp64(labels_true, labels_pred):
    """-> the record MI, H_true, H_pred, EMI, NMI, AMI, n_classes, n_clusters, status"""
    lt, lp = np.asarray(labels_true, np.int32), np.asarray(labels_pred, np.int32)
    N = len(lt)
    _, it, a = np.unique(lt, return_inverse=True, return_counts=True)
    _, ip, b = np.unique(lp, return_inverse=True, return_counts=True)
    R, C = len(a), len(b)
    rec = np.zeros(9)
    rec[6], rec[7] = R, C
    if R * C > MAX_CELLS:
        rec[8] = 1
        return rec
    x = np.arange(N + 1, dtype=np.float64)
    lg = _gammaln(x + 1.0)
    ln = np.zeros(N + 1)
    ln[1:] = np.log(x[1:])
    dN, lnN = float(N), ln[N]
    mi = emi = ht = hp = 0.0
    if R > 1 and C > 1:
        table = np.bincount(it.reshape(-1).astype(np.int64) * C + ip.reshape(-1), minlength=R * C)
        nz = np.flatnonzero(table)
        n = table[nz]
        i, j = nz // C, nz % C
        cn = n / dN
        log_outer = (-np.log((a[i].astype(np.int64) * b[j].astype(np.int64)).astype(np.float64)) + lnN) + lnN
        t = cn * (ln[n] - lnN) + cn * log_outer
        t = np.where(np.abs(t) < EPS, 0.0, t)
        terms = np.zeros(R * C)
        terms[nz] = t
        mi = max(grid_sum(terms), 0.0)
        emi = grid_sum(emi_cells(a, b, N, lg, ln, t_table(N)))
    if R > 1:
        ht = -grid_sum((a / dN) * (ln[a] - lnN))
    if C > 1:
        hp = -grid_sum((b / dN) * (ln[b] - lnN))
    normalizer = (ht + hp) / 2.0
    if R == 1 and C == 1:
        nmi = ami = 1.0
    else:
        nmi = 0.0 if mi == 0.0 else mi / normalizer
        if R == 1 or C == 1:
            ami = 0.0
        else:
            den = normalizer - emi
            den = min(den, -EPS) if den < 0 else max(den, EPS)
            num = mi - emi
            num = min(num, -EPS) if num < 0 else max(num, EPS)
            ami = num / den
    rec[:6] = mi, ht, hp, emi, nmi, ami
    return rec


class NumpyClusterMetricsKernels:
    resident = staticmethod(host_labels)

    def metrics(self, labels_true, labels_pred):
        return cluster_metrics_fp64(labels_true, labels_pred)
