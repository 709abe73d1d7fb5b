"""
PCA on the MI355X — drop-in for the reference's
    from sklearn.decomposition import PCA;  PCA(n_components=50).fit_transform(embeddings)              <- tsne.py
with sklearn 1.7.2's attributes.  Column means (slic_col_stats) and the centred D x D Gram matrix (slic_tsne_gram, products and sums
in double) are computed on the device; the D x D eigendecomposition runs on the host in float64 (D is at most a few thousand); the
projection (X - mean) V is a LinearPlan.rows_forward on the centred rows.  The Gram matrix does not go through the linear weight
gradient: that kernel needs both channel counts in fours and adds in fp32, which at N rows loses the digits explained_variance_
is compared on ("t-SNE and PCA").
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream
from .clustering._device import require_device, resident_rows

GRAM_MAX_D = 8192           # SLIC_TSNE_GRAM_MAX_D


class HipPcaKernels:
    """the device side of PCA.  PCA takes another provider with the same methods through `kernels=` (tests of the host logic pass a
    NumPy one as an ARGUMENT; the product has no other)."""

    def __init__(self):
        require_device("PCA")
        self._plans = {}

    def rows(self, X):
        """fp32 device rows with unit stride inside a row (a device tensor, also a row-strided view, is used in place)"""
        return resident_rows(X, "PCA")

    def col_mean(self, x):
        """float64 host column means (column sums in double on the device)"""
        N, D = x.shape
        _lib.require_device(x)
        cs = torch.empty(2, D, dtype=torch.float64, device=x.device)
        ws = _lib.workspace(_lib.load().slic_col_stats_workspace_bytes(N, D), x.device, "pca_cs")
        call("slic_col_stats", ptr(x), N, D, x.stride(0), ptr(cs[0]), ptr(cs[1]), ptr(ws), stream())
        return cs[0].cpu().numpy() / N

    def gram(self, x, mean):
        """float64 host [D, D]: sum_i (x_i - mean)(x_i - mean)^T"""
        N, D = x.shape
        if D > GRAM_MAX_D:
            raise _lib.SlicError("PCA: D = {} is outside what slic_tsne_gram takes (D <= {})".format(D, GRAM_MAX_D))
        tiles = ((D + 15) // 16) ** 2
        shares = max(1, min(64, 2048 // tiles, (N + 255) // 256))        # row ranges: enough workgroups for a small D
        m = torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float64)).to(x.device)
        part = torch.empty(shares, D, D, dtype=torch.float64, device=x.device)
        G = torch.empty(D, D, dtype=torch.float64, device=x.device)
        call("slic_tsne_gram", ptr(x), N, D, x.stride(0), ptr(m), shares, ptr(part), ptr(G), stream())
        return G.cpu().numpy()

    def project(self, x, mean, components):
        """device [N, n] fp32: (x - mean) components^T; mean [D], components [n, D] host arrays"""
        from .models.conv_plan import LinearPlan
        N, D = x.shape
        n = components.shape[0]
        Dp, npad = (D + 3) // 4 * 4, (n + 3) // 4 * 4
        xc = torch.zeros(N, Dp, dtype=torch.float32, device=x.device)
        xc[:, :D] = x
        m = torch.zeros(Dp, dtype=torch.float32, device=x.device)
        m[:D] = torch.from_numpy(np.ascontiguousarray(mean, dtype=np.float32))
        call("slic_sub_rowvec", ptr(xc), N, Dp, Dp, ptr(m), ptr(xc), Dp, stream())
        w = torch.zeros(npad, Dp, dtype=torch.float32, device=x.device)       # both channel counts in fours: zero columns, zero rows
        w[:n, :D] = torch.from_numpy(np.ascontiguousarray(components, dtype=np.float32))
        key = (Dp, npad, str(x.device))
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = LinearPlan(Dp, npad, x.device)
        return plan.rows_forward(xc, w, fresh=True)[:, :n]

    def to_host(self, y):
        return y.cpu().numpy()


class PCA:
    """sklearn.decomposition.PCA(n_components) for an integer n_components: fit / transform / fit_transform, components_ [n, D],
    mean_ [D], explained_variance_ [n], explained_variance_ratio_ [n] (float64 host arrays; the projected rows are fp32).
    Each component's largest-magnitude loading is positive (sklearn's svd_flip(u_based_decision=False)).
    X: ndarray, CPU tensor, or device tensor (used in place)."""

    def __init__(self, n_components, kernels=None):
        self.n_components = n_components
        self.kernels = kernels

    def _provider(self):
        if self._k is None:
            self._k = HipPcaKernels() if self.kernels is None else self.kernels   # raises SlicError without a gfx950 device
        return self._k

    _k = None

    def _check(self, X):
        shape = tuple(X.shape)
        if len(shape) != 2:
            raise ValueError("PCA expects a 2-D array [n_samples, n_features], got shape {}".format(shape))
        n = self.n_components
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise NotImplementedError("PCA: n_components={!r}; only an integer count is built".format(n))
        if not 1 <= n <= min(shape):
            raise ValueError("n_components={!r} must be between 1 and min(n_samples, n_features)={!r}".format(n, min(shape)))

    def _fit(self, X):
        self._check(X)
        k = self._provider()
        x = k.rows(X)
        N, D = x.shape
        n = int(self.n_components)
        self.mean_ = np.asarray(k.col_mean(x), dtype=np.float64)
        G = np.asarray(k.gram(x, self.mean_), dtype=np.float64)
        w, V = np.linalg.eigh((G + G.T) / 2.0)
        order = np.argsort(w)[::-1]
        w, V = np.maximum(w[order], 0.0), V[:, order].T
        big = np.argmax(np.abs(V), axis=1)
        V = V * np.sign(V[np.arange(D), big])[:, None]
        var = w / max(N - 1, 1)
        total = var.sum()
        self.components_ = V[:n].copy()
        self.explained_variance_ = var[:n].copy()
        self.explained_variance_ratio_ = var[:n] / total if total > 0 else np.zeros(n)
        self.n_samples_, self.n_features_in_ = N, D
        return x

    def fit(self, X):
        self._fit(X)
        return self

    def _transform(self, x, device=False):
        k = self._provider()
        if x.shape[1] != self.n_features_in_:
            raise ValueError("X has {} features, PCA was fitted with {}".format(x.shape[1], self.n_features_in_))
        y = k.project(x, self.mean_, self.components_)
        return y if device else k.to_host(y)

    def transform(self, X, device=False):
        """the projected rows as a host fp32 array [N, n] (device=True: as the provider's resident array)"""
        if not hasattr(self, "components_"):
            raise ValueError("this PCA instance is not fitted yet")
        return self._transform(self._provider().rows(X), device)

    def fit_transform(self, X, device=False):
        return self._transform(self._fit(X), device)
