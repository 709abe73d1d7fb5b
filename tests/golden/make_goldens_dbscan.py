"""Generates tests/golden/dbscan.npz: sklearn 1.7.2's DBSCAN(eps, min_samples, metric='cosine') on small fixtures.

    python tests/golden/make_goldens_dbscan.py

Every case stores X (float32), eps, min_samples, sklearn's labels_ and core_sample_indices_.  No pair of distinct rows has a
float64 cosine distance within 1e-5 of eps (asserted), so a float64 decision and sklearn's float32 one agree on every pair and
the labels must match outright.  The zero-row case pins what sklearn does with a zero row: its radius search of X against itself
zeroes the diagonal, so a zero row is its own neighbour, and it is at distance 1 from every other row (zero rows included).
sklearn is needed here only, not by the tests."""
import os

import numpy as np
import sklearn
from sklearn.cluster import DBSCAN

GAP = 1e-5
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dbscan.npz")


def fp64_distances(X):
    X = X.astype(np.float64)
    n = np.sqrt((X * X).sum(1))
    inv = np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)
    d = np.clip(1.0 - (X @ X.T) * inv[:, None] * inv[None, :], 0.0, 2.0)
    np.fill_diagonal(d, 0.0)
    return d


def blobs(rng, n_blobs, per, D, spread, n_noise):
    cen = rng.standard_normal((n_blobs, D))
    rows = [c + spread * rng.standard_normal((per, D)) for c in cen]
    rows.append(rng.standard_normal((n_noise, D)))
    X = np.concatenate(rows).astype(np.float32)
    return X[rng.permutation(len(X))]


def arc(angles, D, rng):
    """rows at the given angles in a random 2-D plane of R^D, random positive scales (cosine depends on angles only)"""
    Q, _ = np.linalg.qr(rng.standard_normal((D, 2)))
    a = np.asarray(angles, np.float64)
    X = np.cos(a)[:, None] * Q[:, 0] + np.sin(a)[:, None] * Q[:, 1]
    return (X * rng.uniform(0.5, 3.0, (len(a), 1))).astype(np.float32)


def cases():
    rng = np.random.default_rng(20261016)
    out = {}
    X = blobs(rng, 6, 40, 16, 0.12, 30)
    X = np.concatenate([X, X[:5], np.zeros((2, 16), np.float32)])            # exact duplicates (of blob and noise rows), zero rows
    out["blobs16_ms2"] = (X, 0.14, 2)
    out["blobs16_ms3"] = (X, 0.14, 3)
    out["blobs16_ms5"] = (X, 0.05, 5)
    X = blobs(rng, 8, 50, 128, 0.15, 40)
    out["blobs128_ms2"] = (X, 0.14, 2)
    out["blobs128_ms3"] = (X, 0.12, 3)
    # two arcs of cores and rows between them: at eps (theta <= 0.2077 rad) row 0.3 reaches 0.1 (arc A) and 0.5 (arc B) only,
    # so it is a border row of both clusters with min_samples = 4; arc B comes first in row order and is cluster 0
    A = [0.0, 0.02, 0.04, 0.06, 0.08, 0.1]
    B = [0.5, 0.52, 0.54, 0.56, 0.58, 0.6]
    ang = B + [0.3, 1.5, 2.5] + A + [0.8, 1.0]        # 0.8 reaches 0.6 only (a border of B), 1.0 and the others are noise
    X = arc(ang, 8, rng)
    X = np.concatenate([X, np.zeros((1, 8), np.float32), X[7:8]])      # a zero row, a duplicate of a noise row
    out["border_ms4"] = (X, 0.0215, 4)
    out["border_ms3"] = (X, 0.0215, 3)
    X = rng.standard_normal((120, 32)).astype(np.float32)              # near-orthogonal: all noise
    out["noise_ms2"] = (X, 0.14, 2)
    out["single_ms1"] = (rng.standard_normal((1, 16)).astype(np.float32), 0.14, 1)
    out["single_ms2"] = (rng.standard_normal((1, 16)).astype(np.float32), 0.14, 2)
    X = np.concatenate([blobs(rng, 3, 10, 16, 0.1, 10), np.zeros((3, 16), np.float32)])
    out["all_core_ms1"] = (X, 0.14, 1)                                 # every row core; each zero row its own cluster
    out["zero_rows_eps1"] = (X, 1.05, 2)                               # eps > 1: a zero row reaches every row
    return out


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    data = {}
    for name, (X, eps, ms) in cases().items():
        d = fp64_distances(X)
        off = ~np.eye(len(X), dtype=bool)
        assert not np.any(np.abs(d[off] - eps) < GAP), (name, "a pair within 1e-5 of eps")
        m = DBSCAN(eps=eps, min_samples=ms, metric='cosine').fit(X)
        data[name + "__X"] = X
        data[name + "__eps"] = np.float64(eps)
        data[name + "__min_samples"] = np.int64(ms)
        data[name + "__labels"] = m.labels_.astype(np.int32)
        data[name + "__core"] = m.core_sample_indices_.astype(np.int64)
        print("{:16s} N={:4d} D={:3d} eps={} ms={}: {} clusters, {} noise, {} core".format(
            name, len(X), X.shape[1], eps, ms, len(set(m.labels_)) - (1 if -1 in m.labels_ else 0), int((m.labels_ < 0).sum()),
            len(m.core_sample_indices_)))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
