"""float64 restatement of the t-SNE and PCA passes (csrc/tsne.hip, manifold.py, decomposition.py), the test inputs, and the
perplexity search shared with the float32 provider (tsne_cpu_kernels.py).  NumPy only."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)           # sklearn: MACHINE_EPSILON
ULP32 = float(np.finfo(np.float32).eps)         # 2^-23


# ---------------------------------------------------------------- inputs
def blobs(N, D, seed, special=True, outlier=True):
    """N points in 6 Gaussian blobs: centres ~ 4 N(0, 1), rows = centre + N(0, 1), float32.  special: row 1 is a copy of row 0 and
    (outlier) the last row is multiplied by 1e3."""
    rs = np.random.RandomState(seed)
    centres = 4.0 * rs.standard_normal((6, D))
    X = (centres[rs.randint(0, 6, N)] + rs.standard_normal((N, D))).astype(np.float32)
    if special:
        X[1] = X[0]
        if outlier:
            X[-1] *= np.float32(1e3)
    return X


def decaying(N, D, ratio, seed):
    """rows whose column scales decay geometrically (no near-ties in the spectrum), off-centre, float32"""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((N, D)) * ratio ** np.arange(D) + rs.standard_normal(D)).astype(np.float32)


def embedding(N, scale, seed):
    """Y [N, 2] float32 at a scale, with Y[1] = Y[0] (a coincident pair)"""
    Y = (scale * np.random.RandomState(seed).standard_normal((N, 2))).astype(np.float32)
    Y[1] = Y[0]
    return Y


COND_CASES = [(65, 3, 5), (257, 50, 30), (257, 50, 5), (1000, 128, 30)]          # (N, D, perplexity), each with the special rows
FORCE_CASES = [(N, scale, e) for N in (65, 257, 1000) for scale in (1e-4, 1.0, 20.0) for e in (12.0, 1.0)]
PCA_CASES = [(300, 64, 10, 0.85), (1000, 130, 50, 0.93)]                         # (N, D, n, column-scale ratio)
E2E = dict(N=600, D=16, perplexity=30.0, n_init=8)
STEPS_N, STEPS = 257, 20


def cond_key(case):
    return "cond_{}_{}_{}".format(*case)


def force_key(case):
    return "force_{}_{:g}_{:g}".format(*case)


def cond_input(case):
    N, D, _ = case
    return blobs(N, D, 100 + N + D)


def sqdist64(X):
    X = np.asarray(X, dtype=np.float64)
    d = X[:, None, :] - X[None, :, :] if X.shape[0] * X.shape[0] * X.shape[1] <= 4e7 else None
    if d is not None:
        return (d * d).sum(-1)
    out = np.empty((X.shape[0], X.shape[0]))
    for i in range(X.shape[0]):
        t = X[i] - X
        out[i] = (t * t).sum(-1)
    return out


def joint_input(case):
    """P (float32, symmetrised by the float64 restatement) of a blob input for the force tests"""
    N = case[0]
    d2 = sqdist64(blobs(N, 8, 300 + N, outlier=False)).astype(np.float32)
    return joint(search(d2, min(30.0, (N - 1) / 3.0), np.float64, 300, 1e-13)[0]).astype(np.float32)


# ---------------------------------------------------------------- perplexity search
def search(d2, perplexity, dtype, steps, tol):
    """sklearn's _binary_search_perplexity rule, dense case, on distances shifted by the row minimum, every row at once.
    exp and the shifted distances in `dtype`, the row sums in float64.  -> (P [N, N] float64: the row of the last step evaluated,
    beta [N], H [N]: the entropy that step evaluated)"""
    N = d2.shape[0]
    diag = np.eye(N, dtype=bool)
    ds = np.asarray(d2, dtype=dtype)
    dmin = np.where(diag, np.inf, ds).min(axis=1).astype(dtype)
    ds = (ds - dmin[:, None]).astype(dtype)
    ds[diag] = 0
    target = np.log(perplexity)
    beta, bmin, bmax = np.ones(N), np.full(N, -np.inf), np.full(N, np.inf)
    used, H, SP = np.ones(N), np.zeros(N), np.ones(N)
    active = np.ones(N, dtype=bool)

    def rows(idx, b):
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.exp((-b).astype(dtype)[:, None] * ds[idx]).astype(dtype)
        p[diag[idx]] = 0
        return p

    for _ in range(steps):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        used[idx] = beta[idx]
        p = rows(idx, beta[idx])
        sp = p.sum(axis=1, dtype=np.float64)
        sdp = (p.astype(np.float64) * ds[idx].astype(np.float64)).sum(axis=1)
        sp = np.where(sp == 0.0, 1e-8, sp)
        h = np.log(sp) + beta[idx] * (sdp / sp)
        H[idx], SP[idx] = h, sp
        diff = h - target
        done = np.abs(diff) <= tol
        active[idx[done]] = False
        up, dn = idx[(diff > 0) & ~done], idx[(diff <= 0) & ~done]
        bmin[up] = beta[up]
        beta[up] = np.where(np.isinf(bmax[up]), beta[up] * 2.0, (beta[up] + bmax[up]) / 2.0)
        bmax[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(bmin[dn]), beta[dn] / 2.0, (beta[dn] + bmin[dn]) / 2.0)
    P = rows(np.arange(N), used).astype(np.float64) / SP[:, None]
    return P, used, H


def cond_p64(d2, perplexity):
    """the converged float64 search: P [N, N]"""
    return search(np.asarray(d2, dtype=np.float64), perplexity, np.float64, 400, 1e-13)[0]


def entropy(P):
    """-sum p log p of every row, float64"""
    P = np.asarray(P, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(P > 0, P * np.log(P), 0.0)
    return -t.sum(axis=1)


def joint(Pc):
    """(P + P^T) / sum(P + P^T), floored at MACHINE_EPSILON off the diagonal, 0 on it"""
    Pc = np.asarray(Pc, dtype=np.float64)
    S = Pc + Pc.T
    J = np.maximum(S / max(S.sum(), EPS), EPS)
    np.fill_diagonal(J, 0.0)
    return J


# ---------------------------------------------------------------- forces, update, descent
def forces64(P, Y, e):
    """-> grad [N, 2], Z, KL (of e P against w / Z over i != j), S [N] (the absolute-term sum the error is measured against)"""
    P, Y = np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N = Y.shape[0]
    diff = Y[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff * diff).sum(-1))
    off = ~np.eye(N, dtype=bool)
    Z = w[off].sum()
    coef = e * P * w - w * w / Z
    grad = 4.0 * (coef[:, :, None] * diff).sum(axis=1)
    S = 4.0 * ((e * P * w + w * w / Z)[:, :, None] * np.abs(diff)).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(off & (P > 0), e * P * np.log(e * P * Z / w), 0.0).sum()
    return grad, Z, kl, S


def update_rule(Y, upd, gains, grad, momentum, lr, dtype):
    """sklearn's _gradient_descent update in `dtype`: -> (Y, update, gains, gains * grad)"""
    f = dtype
    Y, upd, gains, grad = (np.asarray(a, dtype=f) for a in (Y, upd, gains, grad))
    inc = upd * grad < 0
    gains = np.where(inc, gains + f(0.2), gains * f(0.8)).astype(f)
    gains = np.maximum(gains, f(0.01))
    gg = (grad * gains).astype(f)
    upd = (f(momentum) * upd - f(lr) * gg).astype(f)
    return (Y + upd).astype(f), upd, gains, gg


def descend64(P, Y0, steps, e, momentum, lr):
    Y = np.asarray(Y0, dtype=np.float64)
    upd, gains = np.zeros_like(Y), np.ones_like(Y)
    for _ in range(steps):
        grad = forces64(P, Y, e)[0]
        Y, upd, gains, _ = update_rule(Y, upd, gains, grad, momentum, lr, np.float64)
    return Y


# ---------------------------------------------------------------- trustworthiness (sklearn.manifold.trustworthiness, euclidean)
def trustworthiness(X, Y, n_neighbors):
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N = X.shape[0]
    dX = sqdist64(X)
    np.fill_diagonal(dX, np.inf)
    ind_X = np.argsort(dX, axis=1, kind="stable")
    dY = sqdist64(Y)
    np.fill_diagonal(dY, np.inf)
    ind_Y = np.argsort(dY, axis=1, kind="stable")[:, :n_neighbors]
    inv = np.zeros((N, N), dtype=np.int64)
    inv[np.arange(N)[:, None], ind_X] = np.arange(1, N + 1)
    ranks = inv[np.arange(N)[:, None], ind_Y] - n_neighbors
    t = np.sum(ranks[ranks > 0])
    return 1.0 - t * (2.0 / (N * n_neighbors * (2.0 * N - 3.0 * n_neighbors - 1.0)))


# ---------------------------------------------------------------- PCA
def pca64(X, n):
    """-> (components [n, D], mean [D], explained_variance [n], projected rows [N, n]), float64, sklearn's sign rule"""
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0)
    Xc = X - mean
    w, V = np.linalg.eigh(Xc.T @ Xc)
    order = np.argsort(w)[::-1][:n]
    w, V = w[order], V[:, order].T
    V = V * np.sign(V[np.arange(n), np.argmax(np.abs(V), axis=1)])[:, None]
    return V, mean, w / (X.shape[0] - 1), Xc @ V.T
