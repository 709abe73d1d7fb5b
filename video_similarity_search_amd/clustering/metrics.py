"""
NMI / AMI of two labellings on the MI355X — drop-in for the reference's
    from sklearn.metrics import adjusted_mutual_info_score, normalized_mutual_info_score        <- online_train.py:33, :633-639
with sklearn 1.7.2's values (average_method='arithmetic'; rules in include/slic_hip.h, slic_cluster_metrics).  The whole
computation is one call into csrc/metrics.hip: dense class ids, the contingency table, MI, both entropies, the expected mutual
information (tables of log-gamma values, of logs and of T(x) = sum_{k<x} log1p(-k/N), one exp per (class, cluster, n) term, spread
over the machine) and the two scores,
finished on the device.  What comes back is one record of nine doubles.
"""
import numpy as np
import torch

from .. import _lib
from .._lib import call, ptr, stream

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
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.SlicError("cluster metrics need a gfx950 device (no CPU fallback)")
        if max_cells is not None and not 1 <= int(max_cells) <= MAX_CELLS:
            raise ValueError("max_cells must be in 1 .. {}, got {!r}".format(MAX_CELLS, max_cells))
        self.max_cells = MAX_CELLS if max_cells is None else int(max_cells)

    def resident(self, labels):
        """int32 device labels with unit stride (no copy when they already are); `labels` is an int32 host array or a device tensor"""
        if torch.is_tensor(labels):
            x = labels.detach().to(device="cuda", dtype=torch.int32)
        else:
            x = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
        return x.contiguous()

    def metrics(self, labels_true, labels_pred):
        """-> the record (MI, H_true, H_pred, EMI, NMI, AMI, n_classes, n_clusters, status) as a host float64 array"""
        N = labels_true.shape[0]
        _lib.require_device(labels_true, labels_pred)
        max_cells = min(N * N, self.max_cells)
        nbytes = _lib.load().slic_cluster_metrics_workspace_bytes(N, max_cells)
        if nbytes == 0:
            raise _lib.SlicError("cluster metrics: {} labels are outside what slic_cluster_metrics takes (1 <= N <= {})".format(N, MAX_N))
        ws = _lib.workspace(nbytes, labels_true.device, tag="cluster_metrics")
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
