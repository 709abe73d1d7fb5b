"""
Pair statistics of an embedding on the MI355X: the histogram of the pairwise cosine distances, split into the pairs whose rows share
a label and the pairs that do not — the number behind every distance threshold the clustering ports take (DBSCAN's eps, OPTICS'
max_eps, Agglomerative's distance_threshold; the reference hard-codes them per data set, clustering/cluster_masks.py:50-62, :89) —
and, from the same pass, intra- / inter-class mean and spread, the uniformity of Wang & Isola and, on the host, the verification
numbers of a similarity search (ROC AUC, equal-error rate, TAR at a FAR, the distance below which a share of the pairs is correct).

The whole device side is one call into csrc/pairstats.hip (rules in include/slic_hip.h, slic_pair_stats): the N x N matrix is streamed
through the MFMA ring and never written; what comes back is a table of 2 x bins counts and a record of nine doubles.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream
from .clustering._device import require_device, resident_labels, resident_rows, sized_workspace

MAX_N = 1 << 20             # SLIC_PAIR_STATS_MAX_N, per side
MAX_D = 512
MIN_BINS, MAX_BINS = 8, 4096        # SLIC_PAIR_STATS_MAX_BINS
RECORD = 9                  # SLIC_PAIR_STATS_RECORD: n_diff, n_same, sum d (diff, same), sum d^2 (diff, same), sum e (diff, same), status


class HipPairStatsKernels:
    """the device side: resident rows and labels and the one library call.  The public functions take another provider with the same
    three methods through `kernels=` (tests of the host logic pass a NumPy one as an ARGUMENT; the product has no other)."""

    def __init__(self):
        require_device("pair statistics")

    def resident_rows(self, X):
        """fp32 device rows with unit stride inside a row (a device tensor, also a row-strided view, is used in place)"""
        return resident_rows(X, "pair statistics", dense=False)

    resident_labels = staticmethod(resident_labels)             # int32 device labels with unit stride

    def pair_stats(self, x, x_labels, y, y_labels, bins, t, ignore_label=None):
        """-> (hist int64 [2, bins] (row 0: different label, row 1: same label), record float64 [RECORD]) as host arrays;
        one library call, one read-back"""
        _lib.require_device(x, x_labels, y, y_labels)
        Nx, D = x.shape
        Ny = 0 if y is None else y.shape[0]
        dev = x.device
        ws = sized_workspace("slic_pair_stats_workspace_bytes", (Nx, Ny, D, bins), dev, "pair_stats",
                             "pair statistics: {} x {} rows of D = {} with {} bins are outside what slic_pair_stats takes "
                             "(1 <= N <= {} per side, 1 <= D <= {}, padded rows below 4 GiB)".format(Nx, Ny or Nx, D, bins, MAX_N, MAX_D))
        out = torch.empty(2 * bins + RECORD, dtype=torch.int64, device=dev)           # the counts, then the record's bits
        call("slic_pair_stats", ptr(x), Nx, x.stride(0), ptr(x_labels), ptr(y), Ny, 0 if y is None else y.stride(0), ptr(y_labels),
             D, bins, 0 if ignore_label is None else 1, 0 if ignore_label is None else int(ignore_label), float(t),
             ptr(out), ptr(out[2 * bins:]), ptr(ws), stream())
        host = out.cpu().numpy()
        return host[:2 * bins].reshape(2, bins).copy(), host[2 * bins:].view(np.float64).copy()


def _rows(x, name):
    if torch.is_tensor(x):
        if x.dim() != 2:
            raise ValueError("{} must be 2D [n_samples, n_features]: shape is {}".format(name, tuple(x.shape)))
        if not x.is_floating_point():
            raise ValueError("{} must hold floating-point rows, got {}".format(name, x.dtype))
        if x.is_cuda:
            return x
        x = x.detach().numpy()
    a = np.asarray(x)
    if a.ndim != 2:
        raise ValueError("{} must be 2D [n_samples, n_features]: shape is {}".format(name, a.shape))
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("{} must hold numbers, got dtype {}".format(name, a.dtype))
    return np.ascontiguousarray(a, dtype=np.float32)


def _check_bins_t(bins, t):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not MIN_BINS <= bins <= MAX_BINS or bins & (bins - 1):
        raise ValueError("bins must be a power of two in {} .. {}, got {!r}".format(MIN_BINS, MAX_BINS, bins))
    if not (isinstance(t, (int, float, np.integer, np.floating)) and 0 < float(t) < float("inf")):
        raise ValueError("t must be a positive number, got {!r}".format(t))
    return int(bins), float(t)


def _div(a, b):
    return a / b if b else float("nan")


def _summary(hist, rec, bins, t):
    n_diff, n_same = int(hist[0].sum()), int(hist[1].sum())
    out = {"hist_same": hist[1].astype(np.int64), "hist_diff": hist[0].astype(np.int64), "edges": np.arange(bins + 1) * (2.0 / bins),
           "n_same": n_same, "n_diff": n_diff, "bins": bins, "t": t, "record": np.asarray(rec, dtype=np.float64)}
    for g, name in ((0, "diff"), (1, "same")):
        n = (n_diff, n_same)[g]
        mean = _div(float(rec[2 + g]), n)
        out["mean_" + name] = mean
        out["std_" + name] = math.sqrt(max(float(rec[4 + g]) / n - mean * mean, 0.0)) if n else float("nan")
    n_all = n_same + n_diff
    out["uniformity"] = math.log(float(rec[6] + rec[7]) / n_all) if n_all else float("nan")
    out["uniformity_diff"] = math.log(float(rec[6]) / n_diff) if n_diff else float("nan")
    return out


def pair_statistics(x, x_labels=None, y=None, y_labels=None, bins=256, t=2.0, ignore_label=None, *, kernels=None):
    """The distribution of the pairwise cosine distances d = clip(1 - x^_i . x^_j, 0, 2) (unit rows in fp32; a zero row is at d = 1
    from every row), in `bins` equal bins over [0, 2], split by label: one device call and one small read-back.
        y is None   x against itself: every pair i < j once, no row with itself
        y given     every pair of a row of x and a row of y; labels on both sides or on neither
    Rows: ndarray, CPU tensor, or device tensor (used in place, also a row-strided view).  Labels: as cluster_scores takes them.  A
    pair is "same" iff both rows are labelled and the labels are equal; without labels every pair is "diff".  ignore_label: rows with
    this label (DBSCAN's -1) take part in no pair.  bins: a power of two in 8 .. 4096.  t: the uniformity temperature.
    -> {'hist_same', 'hist_diff': np.int64 [bins]; 'edges': float64 [bins + 1] (bin b holds edges[b] <= d < edges[b + 1], d = 2 in the
        last); 'n_same', 'n_diff': int; 'mean_same', 'mean_diff', 'std_same', 'std_diff' (population std; NaN for an empty group);
        'uniformity' = log mean exp(-t |x^_i - x^_j|^2) over all counted pairs (Wang & Isola; |x^_i - x^_j|^2 = 2 d),
        'uniformity_diff' the same over the different-label pairs; 'bins', 't', 'record' (the device record)}."""
    from .clustering.metrics import _labels
    bins, t = _check_bins_t(bins, t)
    xr = _rows(x, "x")
    yr = None if y is None else _rows(y, "y")
    if y is None and y_labels is not None:
        raise ValueError("y_labels without y")
    if yr is not None and xr.shape[1] != yr.shape[1]:
        raise ValueError("x and y must have the same number of columns: {} vs {}".format(xr.shape[1], yr.shape[1]))
    if xr.shape[0] < 1 or xr.shape[1] < 1 or (yr is not None and yr.shape[0] < 1):
        raise ValueError("pair statistics need at least one row and one column")
    if yr is not None and (x_labels is None) != (y_labels is None):
        raise ValueError("the two-set form takes labels on both sides or on neither")
    lx = None if x_labels is None else _labels(x_labels, "x_labels")
    ly = None if y_labels is None else _labels(y_labels, "y_labels")
    for lab, rows, name in ((lx, xr, "x"), (ly, yr, "y")):
        if lab is not None and lab.shape[0] != rows.shape[0]:
            raise ValueError("Found input variables with inconsistent numbers of samples: {} has {} rows, {}_labels {}".format(
                name, rows.shape[0], name, lab.shape[0]))
    if ignore_label is not None and not -2 ** 31 <= int(ignore_label) <= 2 ** 31 - 1:
        raise ValueError("ignore_label outside int32: {!r}".format(ignore_label))
    k = HipPairStatsKernels() if kernels is None else kernels                   # raises SlicError without a gfx950 device
    hist, rec = k.pair_stats(k.resident_rows(xr), None if lx is None else k.resident_labels(lx),
                             None if yr is None else k.resident_rows(yr), None if ly is None else k.resident_labels(ly),
                             bins, t, ignore_label)
    return _summary(np.asarray(hist), rec, bins, t)


def view_statistics(z1, z2, bins=256, t=2.0, *, kernels=None):
    """Two views of the same N samples (row i of z1 and row i of z2 are a positive pair): the two-set form with labels arange(N) on
    both sides, so the "same" group is the N positive pairs and the "diff" group the N (N - 1) negatives.
    -> {'alignment': 2 * mean_same = mean |z^1_i - z^2_i|^2 (Wang & Isola's alignment loss, alpha = 2); 'uniformity': log mean
        exp(-t |z^1_i - z^2_j|^2) over the negatives ('uniformity_all': over all N^2 pairs); and every other field of
        pair_statistics}.  separation(result) gives the positive-against-negative AUC."""
    a, b = _rows(z1, "z1"), _rows(z2, "z2")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError("the two views must have one shape: {} vs {}".format(tuple(a.shape), tuple(b.shape)))
    ids = np.arange(a.shape[0], dtype=np.int32)
    out = pair_statistics(a, ids, b, ids, bins=bins, t=t, kernels=kernels)
    out["alignment"] = 2.0 * out["mean_same"]
    out["uniformity_all"] = out["uniformity"]
    out["uniformity"] = out["uniformity_diff"]
    return out


def separation(stats, far=(1e-3, 1e-2), precision=(0.9, 0.99)):
    """How well the distance separates same-label from different-label pairs: host arithmetic on the two histograms of
    pair_statistics / view_statistics (exact integers; nothing here touches a device).
    With hs / hd the same / diff counts per bin, ns / nd their totals and edges e_k = 2 k / bins, k = 0 .. bins, the rule
    "accept a pair iff d < e_k" accepts S(k) = sum_{b < k} hs[b] same pairs and F(k) = sum_{b < k} hd[b] diff pairs:
    TAR(k) = S(k) / ns, FAR(k) = F(k) / nd, FRR(k) = 1 - TAR(k).
      auc           P(d_same < d_diff) + P(tie) / 2 over all (same pair, diff pair) couples, two pairs in one bin counting as a tie:
                    sum_b hs[b] (A(b) + hd[b] / 2) / (ns nd), A(b) = diff pairs in bins above b.  NaN when a group is empty.
      auc_bounds    (all ties lost, all ties won) = (sum_b hs[b] A(b), sum_b hs[b] (A(b) + hd[b])) / (ns nd): the AUC of the
                    un-binned fp32 distances lies inside, because binning only hides the order inside a bin.
      eer, eer_edge the first edge k at which |FAR(k) - FRR(k)| is smallest; eer = (FAR(k) + FRR(k)) / 2 there.
      tar_at_far    {f: TAR(k)} at the largest k with FAR(k) <= f (k = 0 always qualifies); edge_at_far {f: e_k} is that edge.
      d_at_precision {p: e_k} for the largest k >= 1 with S(k) + F(k) > 0 and S(k) / (S(k) + F(k)) >= p: below that distance at
                    least a share p of the pairs are same-label — the candidate eps / distance_threshold; None when no edge does."""
    hs = [int(v) for v in np.asarray(stats["hist_same"]).reshape(-1)]
    hd = [int(v) for v in np.asarray(stats["hist_diff"]).reshape(-1)]
    if len(hs) != len(hd) or not hs:
        raise ValueError("hist_same and hist_diff must have one length")
    bins = len(hs)
    edges = [2.0 * k / bins for k in range(bins + 1)]
    ns, nd = sum(hs), sum(hd)
    S, F = [0], [0]
    for b in range(bins):
        S.append(S[-1] + hs[b])
        F.append(F[-1] + hd[b])
    out = {"n_same": ns, "n_diff": nd}
    if ns == 0 or nd == 0:
        nan = float("nan")
        out.update(auc=nan, auc_bounds=(nan, nan), eer=nan, eer_edge=None, tar_at_far={f: nan for f in far},
                   edge_at_far={f: None for f in far})
    else:
        lost = sum(hs[b] * (nd - F[b + 1]) for b in range(bins))
        ties = sum(hs[b] * hd[b] for b in range(bins))
        out["auc"] = (2 * lost + ties) / (2 * ns * nd)
        out["auc_bounds"] = (lost / (ns * nd), (lost + ties) / (ns * nd))
        # |FAR - FRR| = |F nd^-1 - (ns - S) ns^-1| = |F ns - (ns - S) nd| / (ns nd): compared as integers
        k = min(range(bins + 1), key=lambda i: (abs(F[i] * ns - (ns - S[i]) * nd), i))
        out["eer"] = 0.5 * (F[k] / nd + (ns - S[k]) / ns)
        out["eer_edge"] = edges[k]
        out["tar_at_far"], out["edge_at_far"] = {}, {}
        for f in far:
            k = max(i for i in range(bins + 1) if F[i] <= f * nd)
            out["tar_at_far"][f] = S[k] / ns
            out["edge_at_far"][f] = edges[k]
    out["d_at_precision"] = {}
    for p in precision:
        ok = [i for i in range(1, bins + 1) if S[i] + F[i] > 0 and S[i] >= p * (S[i] + F[i])]
        out["d_at_precision"][p] = edges[max(ok)] if ok else None
    return out
