"""NumPy stand-ins for HipTsneKernels (manifold.py) and HipPcaKernels (decomposition.py): every method restated in float32 storage
with the sums the kernels keep in double kept in double.  They drive the same Python drivers on a machine without a device, and
their distance from the float64 restatement (tsne_ref.py) is what the device tests' bounds are multiples of."""
import numpy as np

import tsne_ref as R

f32 = np.float32


class NumpyPcaKernels:
    def rows(self, X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("PCA expects a 2-D array [n_samples, n_features], got shape {}".format(X.shape))
        return X

    def col_mean(self, x):
        return x.sum(axis=0, dtype=np.float64) / x.shape[0]

    def gram(self, x, mean):
        xc = x.astype(np.float64) - np.asarray(mean, dtype=np.float64)
        return xc.T @ xc

    def project(self, x, mean, components):
        xc = (x - np.asarray(mean, dtype=np.float32)).astype(np.float32)
        return xc @ np.asarray(components, dtype=np.float32).T

    def to_host(self, y):
        return np.asarray(y)


class NumpyTsneKernels:
    def __init__(self):
        self.steps = 0              # slic_tsne_step calls
        self.reads = 0              # record read-backs
        self.kl_steps = 0           # steps that asked for the KL pieces

    def rows(self, X):
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("t-SNE expects a 2-D array [n_samples, n_features], got shape {}".format(X.shape))
        return X

    def pca_kernels(self):
        return NumpyPcaKernels()

    def sqdist(self, x):
        """fp32, the direct form, k ascending"""
        N, D = x.shape
        d2 = np.zeros((N, N), dtype=np.float32)
        for k in range(D):
            t = x[:, None, k] - x[None, :, k]
            d2 += t * t
        return d2

    def cond_p(self, d2, perplexity):
        P, beta, self.last_H = R.search(d2, perplexity, np.float32, 100, 1e-5)
        d2[...] = P.astype(np.float32)
        return beta.astype(np.float32)

    def symmetrize(self, P):
        total = 2.0 * P.sum(dtype=np.float64)
        J = np.maximum(((P.astype(np.float64) + P.T.astype(np.float64)) * (1.0 / max(total, R.EPS))).astype(np.float32), f32(R.EPS))
        np.fill_diagonal(J, 0.0)
        P[...] = J
        return P

    def start(self, Y0, P):
        Y = np.array(Y0, dtype=np.float32)
        return {"Y": Y, "update": np.zeros_like(Y), "gains": np.ones_like(Y), "record": np.full(4, np.nan)}

    def forces(self, P, Y, e, want_kl):
        """-> grad [N, 2] fp32, Z, KL: pair terms and the force sums in fp32, Z and the KL pieces summed in float64"""
        N = Y.shape[0]
        dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
        w = (f32(1.0) / (f32(1.0) + (dx * dx + dy * dy))).astype(np.float32)
        off = ~np.eye(N, dtype=bool)
        Z = w.sum(dtype=np.float64) - np.trace(w).astype(np.float64)
        pw, w2 = (f32(e) * P) * w, w * w
        attr = np.stack([(pw * dx).sum(axis=1, dtype=np.float32), (pw * dy).sum(axis=1, dtype=np.float32)], axis=1)
        rep = np.stack([(w2 * dx).sum(axis=1, dtype=np.float32), (w2 * dy).sum(axis=1, dtype=np.float32)], axis=1)
        grad = (f32(4.0) * (attr - rep / f32(Z))).astype(np.float32)
        kl = np.nan
        if want_kl:
            m = off & (P > 0)
            p = P[m]
            plp = (p.astype(np.float64) * np.log(p).astype(np.float64)).sum()
            plw = (p.astype(np.float64) * np.log(w[m]).astype(np.float64)).sum()
            ps = p.sum(dtype=np.float64)
            kl = float(e) * (plp + ps * (np.log(float(e)) + np.log(Z)) - plw)
        return grad, Z, kl

    def step(self, P, st, exaggeration, momentum, learning_rate, want_kl, grad_out=None):
        self.steps += 1
        self.kl_steps += bool(want_kl)
        grad, Z, kl = self.forces(P, st["Y"], exaggeration, want_kl)
        if grad_out is not None:
            grad_out[...] = grad
        st["Y"], st["update"], st["gains"], gg = R.update_rule(st["Y"], st["update"], st["gains"], grad, momentum, learning_rate, np.float32)
        st["record"] = np.array([Z, kl, np.sqrt((gg.astype(np.float64) ** 2).sum()), P.sum(dtype=np.float64) if want_kl else np.nan])

    def record(self, st):
        self.reads += 1
        return st["record"]

    def embedding(self, st):
        return st["Y"]
