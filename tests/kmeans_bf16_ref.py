"""Host emulation of the certified bf16 E-step, shared by tests/test_kmeans_bf16_cpu.py and tests/test_kmeans_bf16_gpu.py:
rows rounded to bf16 (round to nearest even), exact products, fp32 accumulation; the per-pair bound b(i, j); the candidate rule; the
exact scores from the oracle's fmaf chain; and the input generators of both files."""
import numpy as np
import torch


def eps():
    from video_similarity_search_amd import _lib
    return float(_lib.load().slic_kmeans_bf16_eps())


def exact_scores(X, C):
    """s(i, j) = fmaf(-2, dot, cnorm[j]) with the oracle's k-ascending fmaf chain: one oracle E-step per centroid, whose winning score is
    that centroid's column"""
    from oracle import kmeans as ok
    return np.stack([ok.assign(X, C[j:j + 1], with_scores=True)[1] for j in range(C.shape[0])], 1)


def coarse(X, C):
    """-> cs [N, K] (float32), b [N, K] (float64): what km_assign_bf16 computes per pair"""
    from oracle import kmeans as ok
    D = X.shape[1]
    xt, ct = torch.from_numpy(X), torch.from_numpy(C)
    acc = (xt.bfloat16().float() @ ct.bfloat16().float().T).numpy()              # bf16 x bf16 is exact in fp32; fp32 accumulation
    cnorm = ok.row_sqnorm_chain(C)
    cs = (cnorm[None, :].astype(np.float64) - 2.0 * acc.astype(np.float64)).astype(np.float32)     # one rounding, as fmaf(-2, acc, cnorm)
    nx = np.sqrt((X.astype(np.float32) ** 2).sum(1, dtype=np.float32)).astype(np.float64)          # fp32 norms, as the library's
    nc = np.sqrt(cnorm).astype(np.float64)
    absu = D * 2.0 ** -125
    b = nx[:, None] * (nc[None, :] * (2 * eps() + 2.0 ** -21) + absu) + cnorm[None, :].astype(np.float64) * 2.0 ** -22 + absu * (1 + nc[None, :])
    return cs, b


def candidates(cs, b):
    """-> mask [N, K] of the candidate rule, ub [N], lo [N, K]"""
    hi = cs.astype(np.float64) + b
    lo = cs.astype(np.float64) - b
    ub = hi.min(1)
    return lo <= ub[:, None], ub, lo


def blobs(N, K, D, seed=7):
    """separated blobs: rows around K unit directions, centres slightly off them; every row has exactly one candidate"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((K, D))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    X = cent[rng.integers(0, K, N)] + 0.3 * rng.standard_normal((N, D)) / np.sqrt(D)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    C = cent + 0.05 * rng.standard_normal((K, D)) / np.sqrt(D)
    return X.astype(np.float32), C.astype(np.float32)


def gaussian_rows(N, K, D, seed):
    """Gaussian unit rows, centred (the benchmark's data); C = K of the rows"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    X = (X - X.mean(0)).astype(np.float32)
    C = X[rng.choice(N, K, replace=False)].copy()
    return X, C


SHAPES = [(1037, 5, 8), (1037, 33, 104), (4099, 130, 264), (2048, 500, 512)]
