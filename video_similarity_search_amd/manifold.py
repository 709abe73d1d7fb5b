"""
Exact t-SNE on the MI355X — drop-in for the reference's
    from sklearn.manifold import TSNE;  TSNE(n_components=2, perplexity=30).fit_transform(pca_rows)          <- tsne.py
after sklearn 1.7.2's TSNE(method='exact'): the dense N x N matrix P of joint probabilities stays on the device (N <= 65 536: 17 GB),
built once per fit by three passes of csrc/tsne.hip (squared distances, the perplexity search, the symmetrisation), and every
iteration of _gradient_descent is one slic_tsne_step (three launches).  The host reads a four-double record at every 50th iteration
(sklearn's n_iter_check) and at the last.  Rules in include/slic_hip.h, slic_tsne_*.

The one deliberate difference from sklearn: the perplexity search runs on each row's distances shifted by the row's smallest one —
the same P, but a far outlier's row converges where sklearn's underflows and stops short of the perplexity.
"""
import numbers

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream
from .clustering._device import require_device, resident_rows, sized_workspace

MAX_N = 65536               # SLIC_TSNE_MAX_N
RECORD = 4                  # SLIC_TSNE_RECORD
REC_Z, REC_KL, REC_GRAD_NORM, REC_SUM_P = 0, 1, 2, 3
EXPLORATION_MAX_ITER = 250  # sklearn: TSNE._EXPLORATION_MAX_ITER
N_ITER_CHECK = 50           # sklearn: TSNE._N_ITER_CHECK


class HipTsneKernels:
    """the device side of t-SNE: resident rows, P, the embedding and its descent state, one library call per method.  TSNE takes
    another provider with the same methods through `kernels=` (tests of the host logic pass a NumPy one as an ARGUMENT; the product
    has no other)."""

    def __init__(self):
        require_device("t-SNE")

    def rows(self, X):
        """fp32 device rows with unit stride inside a row (a device tensor, also a row-strided view, is used in place)"""
        return resident_rows(X, "t-SNE")

    def pca_kernels(self):
        from .decomposition import HipPcaKernels
        return HipPcaKernels()

    def _workspace(self, N, device):
        return sized_workspace("slic_tsne_workspace_bytes", (N,), device, "tsne",
                               "t-SNE: N = {} is outside what slic_tsne_step takes (2 <= N <= {})".format(N, MAX_N))

    def sqdist(self, x):
        """[N, N] fp32: squared euclidean distances, the direct form"""
        N, D = x.shape
        _lib.require_device(x)
        self._workspace(N, x.device)                                             # the limits, before N x N floats are asked for
        d2 = torch.empty(N, N, dtype=torch.float32, device=x.device)
        call("slic_tsne_sqdist", ptr(x), N, D, x.stride(0), ptr(d2), stream())
        return d2

    def cond_p(self, d2, perplexity):
        """in place: distances -> conditional probabilities; returns beta [N]"""
        N = d2.shape[0]
        _lib.require_device(d2)
        beta = torch.empty(N, dtype=torch.float32, device=d2.device)
        call("slic_tsne_cond_p", ptr(d2), N, float(perplexity), ptr(beta), stream())
        return beta

    def symmetrize(self, P):
        N = P.shape[0]
        _lib.require_device(P)
        call("slic_tsne_symmetrize", ptr(P), N, ptr(self._workspace(N, P.device)), stream())
        return P

    def start(self, Y0, P):
        """the descent state of an initial embedding (host fp32 [N, 2]) beside P: Y, update = 0, gains = 1, the record"""
        dev = P.device
        Y = torch.from_numpy(np.ascontiguousarray(Y0, dtype=np.float32)).to(dev)
        return {"Y": Y, "update": torch.zeros_like(Y), "gains": torch.ones_like(Y),
                "record": torch.full((RECORD,), float("nan"), dtype=torch.float64, device=dev)}

    def step(self, P, st, exaggeration, momentum, learning_rate, want_kl, grad_out=None):
        N = P.shape[0]
        call("slic_tsne_step", ptr(P), N, float(exaggeration), float(momentum), float(learning_rate), 1 if want_kl else 0, ptr(st["Y"]),
             ptr(st["update"]), ptr(st["gains"]), ptr(grad_out), ptr(st["record"]), ptr(self._workspace(N, P.device)), stream())

    def record(self, st):
        """(Z, KL, |gains grad|, sum P) of the last step as a host float64 array: the one read-back"""
        return st["record"].cpu().numpy()

    def embedding(self, st):
        return st["Y"].cpu().numpy()


def _check_random_state(seed):
    """sklearn.utils.check_random_state"""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral) and not isinstance(seed, bool):
        return np.random.RandomState(int(seed))
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError("%r cannot be used to seed a numpy.random.RandomState instance" % seed)


class TSNE:
    """sklearn.manifold.TSNE for n_components=2, method='exact', metric='euclidean': fit / fit_transform, embedding_ [N, 2] (host
    fp32), kl_divergence_, n_iter_ (the index of the last iteration run, as sklearn counts it), learning_rate_.
    The schedule is sklearn's: 250 iterations with P x early_exaggeration at momentum 0.5, then momentum 0.8 up to max_iter;
    learning_rate='auto' is max(N / early_exaggeration / 4, 50); at every 50th iteration the descent stops when the KL divergence has
    not improved for n_iter_without_progress iterations or |gains grad| <= min_grad_norm.
    init: 'pca' (decomposition.PCA, scaled so that the first column has standard deviation 1e-4), 'random'
    (1e-4 * RandomState(random_state).standard_normal) or an array [N, 2].
    X: ndarray, CPU tensor, or device tensor (used in place)."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric='euclidean', init='pca', random_state=None, method='exact',
                 kernels=None):
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.metric = metric
        self.init = init
        self.random_state = random_state
        self.method = method
        self.kernels = kernels

    def _check(self, shape):
        if self.n_components != 2:
            raise NotImplementedError("n_components={!r}: the force kernel is written for two dimensions; 3 is not built".format(
                self.n_components))
        if self.method != 'exact':
            raise NotImplementedError("method={!r}: only the exact method (dense P on the device) is built; Barnes-Hut is not".format(
                self.method))
        if self.metric != 'euclidean':
            raise NotImplementedError("metric={!r}: only 'euclidean' is built".format(self.metric))
        if len(shape) != 2:
            raise ValueError("TSNE expects a 2-D array [n_samples, n_features], got shape {}".format(tuple(shape)))
        if not self.perplexity > 0:
            raise ValueError("perplexity must be positive, got {!r}".format(self.perplexity))
        if self.perplexity >= shape[0]:
            raise ValueError("perplexity ({}) must be less than n_samples ({})".format(self.perplexity, shape[0]))
        if self.early_exaggeration < 1.0:
            raise ValueError("early_exaggeration must be at least 1, but is {}".format(self.early_exaggeration))
        if self.max_iter < EXPLORATION_MAX_ITER:
            raise ValueError("max_iter must be at least {}".format(EXPLORATION_MAX_ITER))
        if not (self.learning_rate == 'auto' or (isinstance(self.learning_rate, numbers.Real) and self.learning_rate > 0)):
            raise ValueError("learning_rate must be 'auto' or a positive number, got {!r}".format(self.learning_rate))
        if isinstance(self.init, str):
            if self.init not in ('pca', 'random'):
                raise ValueError("init must be 'pca', 'random' or an array, got {!r}".format(self.init))
        elif tuple(np.shape(self.init)) != (shape[0], 2):
            raise ValueError("init must have shape ({}, 2), got {}".format(shape[0], tuple(np.shape(self.init))))

    def _initial(self, k, x):
        if not isinstance(self.init, str):
            init = self.init.detach().cpu().numpy() if torch.is_tensor(self.init) else np.asarray(self.init)
            return np.ascontiguousarray(init, dtype=np.float32)
        rs = _check_random_state(self.random_state)
        if self.init == 'random':
            return 1e-4 * rs.standard_normal(size=(x.shape[0], 2)).astype(np.float32)
        from .decomposition import PCA
        emb = PCA(n_components=2, kernels=k.pca_kernels()).fit_transform(x).astype(np.float32, copy=False)
        return (emb / np.std(emb[:, 0]) * 1e-4).astype(np.float32)

    def _descend(self, k, P, st, it, max_iter, momentum, exaggeration, n_iter_without_progress):
        """sklearn's _gradient_descent from iteration `it`: -> (KL of the last iteration that computed it, last iteration index)"""
        error = np.finfo(float).max
        best_error = np.finfo(float).max
        best_iter = i = it
        for i in range(it, max_iter):
            check = (i + 1) % N_ITER_CHECK == 0
            want = check or i == max_iter - 1
            k.step(P, st, exaggeration, momentum, self.learning_rate_, want)
            if want:
                rec = k.record(st)
                error = float(rec[REC_KL])
            if check:
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > n_iter_without_progress:
                    break
                if rec[REC_GRAD_NORM] <= self.min_grad_norm:
                    break
        return error, i

    def _fit(self, X):
        self._check(tuple(X.shape))
        k = HipTsneKernels() if self.kernels is None else self.kernels          # raises SlicError without a gfx950 device
        x = k.rows(X)
        N = x.shape[0]
        self.learning_rate_ = (max(N / self.early_exaggeration / 4, 50) if self.learning_rate == 'auto' else float(self.learning_rate))
        P = k.sqdist(x)
        k.cond_p(P, self.perplexity)
        k.symmetrize(P)
        st = k.start(self._initial(k, x), P)
        kl, it = self._descend(k, P, st, 0, EXPLORATION_MAX_ITER, 0.5, self.early_exaggeration, EXPLORATION_MAX_ITER)
        # (sklearn enters the second stage even when no iteration is left, max_iter = 250, and then reports the untouched
        # initial error, the largest float, as kl_divergence_; here the first stage's values stand)
        if it + 1 < self.max_iter:
            kl, it = self._descend(k, P, st, it + 1, self.max_iter, 0.8, 1.0, self.n_iter_without_progress)
        self.n_iter_ = it
        self.kl_divergence_ = kl
        self.embedding_ = np.asarray(k.embedding(st), dtype=np.float32)
        return self.embedding_

    def fit_transform(self, X, y=None):
        return self._fit(X)

    def fit(self, X, y=None):
        self._fit(X)
        return self
