"""
NMI / AMI of two labellings on the MI355X — drop-in for the reference's
    from sklearn.metrics import adjusted_mutual_info_score, normalized_mutual_info_score        <- online_train.py:33, :633-639
with sklearn 1.7.2's values (average_method='arithmetic'; rules in include/slic_hip.h, slic_cluster_metrics).  The whole
computation is one call into csrc/metrics.hip: dense class ids, the contingency table, MI, both entropies, the expected mutual
information (tables of log-gamma values, of logs and of T(x) = sum_{k<x} log1p(-k/N), one exp per (class, cluster, n) term, spread
over the machine) and the two scores,
finished on the device.  What comes back is one record of nine doubles.

The second half of the file is the label-free score: silhouette_samples / silhouette_score / silhouette_report for metric='cosine' and
'sqeuclidean', one call into csrc/silhouette.hip (the rows against the per-cluster means on the MFMA ring; no N x N distances).
"""
import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._device import require_device, resident_labels, resident_rows, sized_workspace

MAX_N = 1 << 24             # SLIC_METRICS_MAX_N
MAX_CELLS = 1 << 26         # SLIC_METRICS_MAX_CELLS: the dense n_classes x n_clusters int32 table
RECORD = 9                  # SLIC_METRICS_RECORD
FIELDS = ("MI", "H_true", "H_pred", "EMI", "NMI", "AMI", "n_classes", "n_clusters", "status")


class HipClusterMetricsKernels:
    """the device side of the metrics: resident labels and the one library call.  The public functions take another provider with
    the same two methods through `kernels=` (tests of the host logic on a GPU-less machine pass a NumPy one as an ARGUMENT; the
    product has no other).
    `max_cells` bounds the dense n_classes x n_clusters int32 table the workspace holds (default and largest: MAX_CELLS).  The class
    counts are not known before the call and the call does not synchronise, so the workspace is sized for the bound, not for the
    data: min(N * N, max_cells) cells, i.e. 256 MiB at the default for N >= 8192, cached between calls like every workspace.  A
    caller who knows its class counts passes a smaller bound (400 classes x 1000 clusters: max_cells=400_000, 1.6 MB)."""

    def __init__(self, max_cells=None):
        require_device("cluster metrics")
        if max_cells is not None and not 1 <= int(max_cells) <= MAX_CELLS:
            raise ValueError("max_cells must be in 1 .. {}, got {!r}".format(MAX_CELLS, max_cells))
        self.max_cells = MAX_CELLS if max_cells is None else int(max_cells)

    resident = staticmethod(resident_labels)                    # int32 device labels with unit stride

    def metrics(self, labels_true, labels_pred):
        """-> the record (MI, H_true, H_pred, EMI, NMI, AMI, n_classes, n_clusters, status) as a host float64 array"""
        N = labels_true.shape[0]
        _lib.require_device(labels_true, labels_pred)
        max_cells = min(N * N, self.max_cells)
        ws = sized_workspace("slic_cluster_metrics_workspace_bytes", (N, max_cells), labels_true.device, "cluster_metrics",
                             "cluster metrics: {} labels are outside what slic_cluster_metrics takes (1 <= N <= {})".format(N, MAX_N))
        rec = torch.empty(RECORD, dtype=torch.float64, device=labels_true.device)
        call("slic_cluster_metrics", ptr(labels_true), ptr(labels_pred), N, max_cells, ptr(rec), ptr(ws), stream())
        return rec.cpu().numpy()


def _labels(x, name):
    """a 1-D labelling as a host int32 array, or as the device tensor it already is (int32 / int64 / ... checked against int32)"""
    if torch.is_tensor(x):
        if x.dim() != 1:
            raise ValueError("{} must be 1D: shape is {}".format(name, tuple(x.shape)))
        if x.is_floating_point() or x.is_complex():
            raise ValueError("{} must hold integer labels, got {}".format(name, x.dtype))
        if x.is_cuda:
            if x.dtype not in (torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool) and x.numel():
                lo, hi = int(x.min()), int(x.max())
                if lo < -2 ** 31 or hi > 2 ** 31 - 1:
                    raise ValueError("{} holds values outside int32 ({} .. {})".format(name, lo, hi))
            return x
        x = x.detach().numpy()
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError("{} must be 1D: shape is {}".format(name, a.shape))
    if a.dtype == np.bool_:
        a = a.astype(np.int32)
    if a.size == 0:
        return np.zeros(0, np.int32)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("{} must hold integer labels, got dtype {}".format(name, a.dtype))
    lo, hi = int(a.min()), int(a.max())
    if lo < -2 ** 31 or hi > 2 ** 31 - 1:
        raise ValueError("{} holds values outside int32 ({} .. {})".format(name, lo, hi))
    return np.ascontiguousarray(a, dtype=np.int32)


def cluster_scores(labels_true, labels_pred, kernels=None, max_cells=None):
    """one library call -> {'NMI', 'AMI', 'MI', 'EMI', 'H_true', 'H_pred': float, 'n_classes', 'n_clusters': int}.
    labels: list, ndarray, CPU tensor, or device tensor (used in place); any int32 values, -1 a class like any other.
    max_cells: an upper bound on n_classes * n_clusters for the device table (HipClusterMetricsKernels); more classes than the
    bound admits raise SlicError."""
    lt, lp = _labels(labels_true, "labels_true"), _labels(labels_pred, "labels_pred")
    if lt.shape[0] != lp.shape[0]:
        raise ValueError("Found input variables with inconsistent numbers of samples: [{}, {}]".format(lt.shape[0], lp.shape[0]))
    if lt.shape[0] < 1:
        raise ValueError("cluster metrics need at least one label")
    k = HipClusterMetricsKernels(max_cells) if kernels is None else kernels     # raises SlicError without a gfx950 device
    rec = np.asarray(k.metrics(k.resident(lt), k.resident(lp)), dtype=np.float64)
    out = dict(zip(FIELDS, (float(v) for v in rec)))
    out["n_classes"], out["n_clusters"] = int(out["n_classes"]), int(out["n_clusters"])
    if out.pop("status") != 0:
        raise _lib.SlicError("cluster metrics: {} classes x {} clusters exceed the dense contingency table of "
                             "slic_cluster_metrics ({} cells)".format(out["n_classes"], out["n_clusters"], getattr(k, "max_cells", MAX_CELLS)))
    return out


def normalized_mutual_info_score(labels_true, labels_pred, kernels=None):
    """sklearn.metrics.normalized_mutual_info_score(labels_true, labels_pred) (average_method='arithmetic')"""
    return cluster_scores(labels_true, labels_pred, kernels=kernels)["NMI"]


def adjusted_mutual_info_score(labels_true, labels_pred, kernels=None):
    """sklearn.metrics.adjusted_mutual_info_score(labels_true, labels_pred) (average_method='arithmetic')"""
    return cluster_scores(labels_true, labels_pred, kernels=kernels)["AMI"]


# ---- silhouette coefficient from per-cluster row sums (csrc/silhouette.hip; contract in include/slic_hip.h, slic_silhouette) ----
SILHOUETTE_METRICS = {"cosine": 0, "sqeuclidean": 1}        # SLIC_SILHOUETTE_COSINE / _SQEUCLIDEAN
SILHOUETTE_MAX_D = 512                                      # SLIC_SILHOUETTE_MAX_D
SILHOUETTE_RECORD = 4                                       # mean s, clusters, rows scored, status
SILHOUETTE_UNDEFINED, SILHOUETTE_TOO_MANY = 1, 2            # status values


class HipSilhouetteKernels:
    """the device side of the silhouette: resident rows and labels and the one library call.  The public functions take another
    provider with the same methods through `kernels=` (tests of the host logic pass a NumPy one as an ARGUMENT; the product has no
    other).  `max_clusters` bounds the number of clusters the workspace admits (default and largest: N - 1): the count is found on
    the device and the call does not synchronise, so the [max_clusters, D] fp32 matrix of cluster means is sized by the bound."""

    def __init__(self, max_clusters=None):
        require_device("the silhouette")
        if max_clusters is not None and int(max_clusters) < 2:
            raise ValueError("max_clusters must be at least 2, got {!r}".format(max_clusters))
        self.max_clusters = None if max_clusters is None else int(max_clusters)

    def resident_rows(self, X):
        """fp32 device rows with unit stride inside a row (a device tensor, also a row-strided view, is used in place)"""
        return resident_rows(X, "the silhouette")

    resident_labels = staticmethod(resident_labels)             # int32 device labels with unit stride

    def take(self, x, idx):
        """rows idx (a host int64 array) of a resident array"""
        return x[torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(x.device)]

    def n_labels(self, labels):
        return int(torch.unique(labels).numel())

    def silhouette(self, X, labels, metric, ignore_label=None, rows=True, clusters=True):
        """-> {'record': float64 [4], 's', 'a', 'b': float32 [N], 'nearest': int32 [N] (rows=True), 'cluster_mean': float64 [K],
        'cluster_label': int32 [K] (clusters=True)}, host arrays; one library call, one read-back"""
        N, D = X.shape
        _lib.require_device(X, labels)
        kmax = N - 1 if self.max_clusters is None else min(self.max_clusters, N - 1)
        dev = X.device
        ws = sized_workspace("slic_silhouette_workspace_bytes", (N, D, kmax), dev, "silhouette",
                             "silhouette: N = {}, D = {} are outside what slic_silhouette takes (3 <= N <= {}, 1 <= D <= {})".format(
                                 N, D, MAX_N, SILHOUETTE_MAX_D))
        rec = torch.empty(SILHOUETTE_RECORD, dtype=torch.float64, device=dev)
        f = torch.empty((3, N), dtype=torch.float32, device=dev) if rows else None
        near = torch.empty(N, dtype=torch.int32, device=dev) if rows else None
        cm = torch.empty(kmax, dtype=torch.float64, device=dev) if clusters else None
        cl = torch.empty(kmax, dtype=torch.int32, device=dev) if clusters else None
        call("slic_silhouette", ptr(X), N, D, X.stride(0), ptr(labels), metric, 0 if ignore_label is None else 1,
             0 if ignore_label is None else int(ignore_label), kmax, ptr(f[0]) if rows else None, ptr(f[1]) if rows else None,
             ptr(f[2]) if rows else None, ptr(near), ptr(rec), ptr(cm), ptr(cl), ptr(ws), stream())
        out = {"record": rec.cpu().numpy(), "max_clusters": kmax}
        if rows:
            fh = f.cpu().numpy()
            out.update(s=fh[0], a=fh[1], b=fh[2], nearest=near.cpu().numpy())
        if clusters:
            k = int(out["record"][1]) if out["record"][3] == 0 else 0
            out.update(cluster_mean=cm[:k].cpu().numpy(), cluster_label=cl[:k].cpu().numpy())
        return out


def _check_random_state(seed):
    """sklearn.utils.check_random_state"""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        return np.random.RandomState(int(seed))
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError("%r cannot be used to seed a numpy.random.RandomState instance" % seed)


def _rows(X):
    """rows as a host fp32 array [N, D], or as the device tensor they already are"""
    if torch.is_tensor(X):
        if X.dim() != 2:
            raise ValueError("X must be 2D: shape is {}".format(tuple(X.shape)))
        if not X.is_floating_point():
            raise ValueError("X must hold floating-point rows, got {}".format(X.dtype))
        if X.is_cuda:
            return X
        X = X.detach().numpy()
    a = np.asarray(X)
    if a.ndim != 2:
        raise ValueError("X must be 2D: shape is {}".format(a.shape))
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise ValueError("X must hold numbers, got dtype {}".format(a.dtype))
    return np.ascontiguousarray(a, dtype=np.float32)


def _silhouette(X, labels, metric, ignore_label, kernels, rows, clusters, sample_size=None, random_state=None):
    if metric == "euclidean":
        raise NotImplementedError("metric='euclidean' has no cluster-sum identity: it needs a streamed N x N pass, which is not "
                                  "built; 'cosine' and 'sqeuclidean' are")
    if metric == "precomputed":
        raise NotImplementedError("metric='precomputed' needs the N x N matrix this implementation exists to avoid")
    if metric not in SILHOUETTE_METRICS:
        raise ValueError("metric={!r}: 'cosine' or 'sqeuclidean'".format(metric))
    x, lab = _rows(X), _labels(labels, "labels")
    if x.shape[0] != lab.shape[0]:
        raise ValueError("Found input variables with inconsistent numbers of samples: [{}, {}]".format(x.shape[0], lab.shape[0]))
    if x.shape[1] < 1:
        raise ValueError("X has no columns")
    if ignore_label is not None and not -2 ** 31 <= int(ignore_label) <= 2 ** 31 - 1:
        raise ValueError("ignore_label outside int32: {!r}".format(ignore_label))
    k = HipSilhouetteKernels() if kernels is None else kernels                  # raises SlicError without a gfx950 device
    x, lab = k.resident_rows(x), k.resident_labels(lab)
    if sample_size is not None:
        idx = _check_random_state(random_state).permutation(x.shape[0])[:sample_size]
        x, lab = k.take(x, idx), k.take(lab, idx)
    N = x.shape[0]
    if N < 3:                                                                   # no count of clusters is inside 2 .. N - 1
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % (k.n_labels(lab) if N else 0))
    out = k.silhouette(x, lab, SILHOUETTE_METRICS[metric], ignore_label, rows=rows, clusters=clusters)
    status = int(out["record"][3])
    if status == SILHOUETTE_UNDEFINED:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % int(out["record"][1]))
    if status != 0:
        raise _lib.SlicError("silhouette: more than max_clusters = {} clusters".format(out.get("max_clusters")))
    return out


def silhouette_samples(X, labels, *, metric='cosine', ignore_label=None, return_parts=False, kernels=None):
    """sklearn.metrics.silhouette_samples(X, labels, metric=metric) for metric 'cosine' or 'sqeuclidean', as a host fp32 array [N]:
    one N x K x D contraction of the rows against the cluster means (csrc/silhouette.hip), no N x N distances.
    X: ndarray, CPU tensor, or device tensor (used in place); labels as cluster_scores takes them.  ignore_label: rows with this
    label (DBSCAN's -1) take no part and come back as NaN.  return_parts: (s, a, b, nearest_label) — the mean distance to the own
    cluster, to the nearest other cluster, and that cluster's label."""
    out = _silhouette(X, labels, metric, ignore_label, kernels, True, False)
    return (out["s"], out["a"], out["b"], out["nearest"]) if return_parts else out["s"]


def silhouette_score(X, labels, *, metric='cosine', sample_size=None, random_state=None, ignore_label=None, kernels=None):
    """sklearn.metrics.silhouette_score: the mean of silhouette_samples (taken on the device in float64, in a fixed order).
    sample_size / random_state as sklearn: check_random_state(random_state).permutation(N)[:sample_size]."""
    return float(_silhouette(X, labels, metric, ignore_label, kernels, False, False, sample_size, random_state)["record"][0])


def silhouette_report(X, labels, *, metric='cosine', sample_size=None, random_state=None, ignore_label=None, kernels=None):
    """-> {'score': float, 'per_cluster': {label: mean s of the cluster}, 'n_clusters': int, 'n_rows': int (rows scored)}"""
    out = _silhouette(X, labels, metric, ignore_label, kernels, False, True, sample_size, random_state)
    rec = out["record"]
    return {"score": float(rec[0]), "per_cluster": {int(l): float(m) for l, m in zip(out["cluster_label"], out["cluster_mean"])},
            "n_clusters": int(rec[1]), "n_rows": int(rec[2])}
