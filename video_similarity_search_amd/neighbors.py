"""
k-nearest-neighbour search and classification on the MI355X, with sklearn 1.7.2's names and results:

    from sklearn.neighbors import NearestNeighbors, KNeighborsClassifier   ->   from video_similarity_search_amd.neighbors import ...

NearestNeighbors is a thin layer over evaluate.cosine_topk / euclidean_topk (the fused GEMM + exact top-k of csrc/topk.hip).
KNeighborsClassifier adds ONE launch of slic_knn_vote (csrc/knn.hip) on the [Nq, k] tables the search leaves on the device: the class
scores are summed in rank order in float32 without atomics, the lowest class wins a tie as sklearn's argmax does.  weights='uniform' and
'distance' are sklearn's; 'softmax' is the k-NN monitor of InstDisc / MoCo / DINO, w = exp(-d / temperature) up to a per-query factor.

Gallery rows, labels and results stay device tensors; `predict` and `score` return what sklearn returns.  What is not built raises with
the reason (regression, radius neighbours, 'precomputed', callable weights, k beyond the search's 88: DESIGN.md section 7j).

The public classes take `kernels=`: another provider with HipKnnKernels' methods (the CPU suite drives the host logic with a NumPy one).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

MAX_K = 88                  # TK_KMAX of the searches (csrc/topk.hip); the vote and the ranked metrics themselves take k <= 1024
MAX_CLASSES = 4096          # SLIC_KNN_MAX_CLASSES
MAX_TOP = 8                 # SLIC_KNN_MAX_TOP
MAX_CUTS = 8                # SLIC_KNN_MAX_CUTS
WEIGHTS = {"uniform": 0, "distance": 1, "softmax": 2}       # SLIC_KNN_UNIFORM / _DISTANCE / _SOFTMAX
METRICS = ("cosine", "euclidean")


class HipKnnKernels(object):
    """the device side: the search, resident labels, the two library calls of csrc/knn.hip, and the read-back.  `reads` counts the
    device-to-host copies made through `read`."""

    def __init__(self):
        if not torch.cuda.is_available():
            raise _lib.SlicError("k-NN needs a gfx950 device (no CPU fallback)")
        _lib.load()
        self.reads = 0

    def rows(self, x):
        """fp32 device rows [N, D]"""
        from .evaluate import _dev
        return _dev(x)

    def labels(self, labels):
        """int64 device labels [N]"""
        from .evaluate import _labels_dev
        return _labels_dev(labels, torch.device("cuda"))

    def search(self, x, y, k, dist_metric, precision="fp32"):
        """(indices [Nq, k] int32, distances [Nq, k] fp32) of the k nearest rows of y (None: of x itself, diagonal excluded)"""
        from .evaluate import _topk_search
        return _topk_search(dist_metric, precision)(x, y, k=k)

    def vote(self, idx, dist, g_labels, n_classes, mode, temperature, n_top, want_proba):
        """slic_knn_vote -> (proba [Nq, C] or None, pred [Nq, n_top] int32 or None, score [Nq, n_top] or None)"""
        _lib.require_device(idx, dist, g_labels)
        idx = idx.to(torch.int32).contiguous()
        dist = None if dist is None else dist.to(torch.float32).contiguous()
        Nq, k = idx.shape
        proba = torch.empty(Nq, n_classes, dtype=torch.float32, device=idx.device) if want_proba else None
        pred = torch.empty(Nq, n_top, dtype=torch.int32, device=idx.device) if n_top else None
        score = torch.empty(Nq, n_top, dtype=torch.float32, device=idx.device) if n_top else None
        call("slic_knn_vote", ptr(idx), ptr(dist), Nq, k, ptr(g_labels), g_labels.shape[0], int(n_classes), int(mode), float(temperature),
             int(n_top), ptr(proba), ptr(pred), ptr(score), stream())
        return proba, pred, score

    def ranked(self, idx, q_labels, g_labels, n_rel, ks):
        """slic_retrieval_ranked -> (per_query [Nq, n_ks, 3] float64, rr [Nq] float64, record [3 n_ks + 2] float64) on the device"""
        _lib.require_device(idx, q_labels, g_labels, n_rel)
        idx = idx.to(torch.int32).contiguous()
        n_rel = n_rel.to(torch.int32).contiguous()
        Nq, k = idx.shape
        cuts = (ctypes.c_int32 * len(ks))(*[int(v) for v in ks])
        per_query = torch.empty(Nq, len(ks), 3, dtype=torch.float64, device=idx.device)
        rr = torch.empty(Nq, dtype=torch.float64, device=idx.device)
        record = torch.empty(3 * len(ks) + 2, dtype=torch.float64, device=idx.device)
        call("slic_retrieval_ranked", ptr(idx), Nq, k, ptr(q_labels), ptr(g_labels), g_labels.shape[0], ptr(n_rel), cuts, len(ks),
             ptr(per_query), ptr(rr), ptr(record), stream())
        return per_query, rr, record

    def read(self, t):
        self.reads += 1
        return t.cpu().numpy()


def check_vote_sizes(who, k, n_classes, n_top=1):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError("{}: n_neighbors = {} is outside 1 .. {} (the exact top-k search stops at {}; a larger k needs a larger-k "
                         "search)".format(who, k, MAX_K, MAX_K))
    if not 1 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError("{}: {} classes; slic_knn_vote keeps one wave's class scores in LDS and takes 1 .. {}".format(
            who, n_classes, MAX_CLASSES))
    if not 0 <= int(n_top) <= MAX_TOP:
        raise ValueError("{}: the {} best classes were asked for; slic_knn_vote ranks at most {}".format(who, n_top, MAX_TOP))


def _check_metric(who, metric):
    if callable(metric) or metric not in METRICS:
        raise NotImplementedError("{}: metric={!r}: only 'cosine' and 'euclidean' are built (the two exact top-k searches); "
                                  "'precomputed', minkowski with p and callables are not".format(who, metric))


class NearestNeighbors(object):
    """sklearn.neighbors.NearestNeighbors(n_neighbors=5, metric='cosine'): fit + kneighbors, brute force on the device."""

    def __init__(self, n_neighbors=5, *, radius=None, algorithm='auto', metric='cosine', p=None, metric_params=None, n_jobs=None,
                 precision="fp32", kernels=None):
        self.n_neighbors, self.radius, self.algorithm, self.metric, self.p = n_neighbors, radius, algorithm, metric, p
        self.metric_params, self.n_jobs, self.precision, self.kernels = metric_params, n_jobs, precision, kernels

    def _check_params(self):
        who = type(self).__name__
        _check_metric(who, self.metric)
        if self.algorithm not in ('auto', 'brute'):
            raise NotImplementedError("{}: algorithm={!r}: the search is brute force on the device ('auto' or 'brute'); trees are not "
                                      "built".format(who, self.algorithm))
        if self.p is not None:
            raise NotImplementedError("{}: p={!r}: the Minkowski family is not built; metric='euclidean' is p = 2".format(who, self.p))
        if self.radius is not None:
            raise NotImplementedError("{}: radius neighbours are not built".format(who))
        if self.metric_params is not None:
            raise NotImplementedError("{}: metric_params are not built".format(who))
        from .evaluate import _check_precision
        _check_precision(self.precision)
        if self.precision != "fp32" and self.metric != "cosine":
            raise ValueError("{}: precision={!r} needs metric='cosine' (the certified bf16 candidate search rests on unit rows)".format(
                who, self.precision))
        self._check_k(self.n_neighbors)

    def _check_k(self, k):
        if not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("Expected n_neighbors > 0. Got {!r}".format(k))
        if k > MAX_K:
            raise ValueError("{}: n_neighbors = {} is beyond the {} of the exact top-k search (a larger k needs a larger-k "
                             "search)".format(type(self).__name__, k, MAX_K))

    def fit(self, X, y=None):
        self._check_params()
        self._K = HipKnnKernels() if self.kernels is None else self.kernels       # raises SlicError without a gfx950 device
        self._fit_X = self._K.rows(X)
        if self._fit_X.dim() != 2:
            raise ValueError("Expected 2D array, got shape {}".format(tuple(self._fit_X.shape)))
        self.n_samples_fit_, self.n_features_in_ = int(self._fit_X.shape[0]), int(self._fit_X.shape[1])
        self.effective_metric_ = self.metric
        return self

    def _search(self, X, n_neighbors):
        if not hasattr(self, "_fit_X"):
            raise RuntimeError("This {} instance is not fitted yet. Call 'fit' first.".format(type(self).__name__))
        k = self.n_neighbors if n_neighbors is None else n_neighbors
        self._check_k(k)
        n_avail = self.n_samples_fit_ - (1 if X is None else 0)
        if k > n_avail:
            raise ValueError("Expected n_neighbors <= n_samples_fit, but n_neighbors = {}, n_samples_fit = {}, n_samples = {}".format(
                k, n_avail, self.n_samples_fit_ if X is None else len(X)))
        if X is None:
            return self._K.search(self._fit_X, None, int(k), self.metric, self.precision)
        return self._K.search(self._K.rows(X), self._fit_X, int(k), self.metric, self.precision)

    def kneighbors(self, X=None, n_neighbors=None, return_distance=True):
        """sklearn's order: (distances [Nq, k] fp32, indices [Nq, k] int32), device tensors; X=None searches the fitted rows, none of
        them its own neighbour."""
        idx, dist = self._search(X, n_neighbors)
        return (dist, idx) if return_distance else idx


class KNeighborsClassifier(NearestNeighbors):
    """sklearn.neighbors.KNeighborsClassifier with weights 'uniform' | 'distance' | 'softmax' (temperature) and metric 'cosine' |
    'euclidean'.  classes_ and n_samples_fit_ as sklearn's; arbitrary integer labels are mapped through classes_."""

    def __init__(self, n_neighbors=5, *, weights='uniform', algorithm='auto', p=None, metric='cosine', metric_params=None, n_jobs=None,
                 temperature=0.07, precision="fp32", kernels=None):
        super().__init__(n_neighbors, algorithm=algorithm, metric=metric, p=p, metric_params=metric_params, n_jobs=n_jobs,
                         precision=precision, kernels=kernels)
        self.weights, self.temperature = weights, temperature

    def _check_params(self):
        super()._check_params()
        if callable(self.weights):
            raise NotImplementedError("KNeighborsClassifier: callable weights are not built; the vote kernel knows 'uniform', "
                                      "'distance' and 'softmax'")
        if self.weights not in WEIGHTS:
            raise ValueError("weights must be 'uniform', 'distance' or 'softmax', got {!r}".format(self.weights))
        if self.weights == 'softmax' and not self.temperature > 0:
            raise ValueError("temperature must be positive, got {!r}".format(self.temperature))

    def fit(self, X, y):
        super().fit(X)
        if torch.is_tensor(y):
            if y.is_floating_point():
                raise ValueError("KNeighborsClassifier: y must hold integer class labels, got {} (regression is not built)".format(y.dtype))
            classes, inverse = torch.unique(y.detach().reshape(-1), sorted=True, return_inverse=True)
            self.classes_ = classes.cpu().numpy()
        else:
            y = np.asarray(y).reshape(-1)
            if not (np.issubdtype(y.dtype, np.integer) or y.dtype == np.bool_):
                raise ValueError("KNeighborsClassifier: y must hold integer class labels, got dtype {} (regression is not built)".format(
                    y.dtype))
            self.classes_, inverse = np.unique(y, return_inverse=True)
        if inverse.shape[0] != self.n_samples_fit_:
            raise ValueError("Found input variables with inconsistent numbers of samples: [{}, {}]".format(
                self.n_samples_fit_, inverse.shape[0]))
        if len(self.classes_) > MAX_CLASSES:
            raise ValueError("KNeighborsClassifier: {} classes; slic_knn_vote keeps one wave's class scores in LDS and takes at most "
                             "{}".format(len(self.classes_), MAX_CLASSES))
        self._y = self._K.labels(inverse)
        return self

    def _vote(self, X, n_top, want_proba):
        idx, dist = self._search(X, None)
        return self._K.vote(idx, dist, self._y, len(self.classes_), WEIGHTS[self.weights], self.temperature, n_top, want_proba)

    def predict_proba(self, X=None):
        """[Nq, n_classes] fp32 on the device, columns in classes_ order; X=None: leave-one-out over the fitted rows"""
        return self._vote(X, 0, True)[0]

    def predict(self, X=None):
        """np.ndarray [Nq] of the labels' dtype, as sklearn returns it; X=None: leave-one-out over the fitted rows"""
        position = self._vote(X, 1, False)[1][:, 0]
        return self.classes_[self._K.read(position)]

    def score(self, X, y):
        """mean accuracy of predict(X) against y"""
        y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
        return float(np.mean(self.predict(X) == y.reshape(-1)))
