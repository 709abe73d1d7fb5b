"""Generates tests/golden/agglomerative.npz: sklearn 1.7.2's
    AgglomerativeClustering(n_clusters=None, linkage='average', distance_threshold=t, metric='cosine')
on small fixtures (the reference's affinity= spelling no longer exists in that sklearn).

    python tests/golden/make_goldens_agglomerative.py

Every case stores X (float32), t, and sklearn's labels_ renumbered canonically: clusters 0 .. C-1 in order of first appearance, the
numbering clustering/agglomerative.py documents (sklearn's own numbers come from node ids of the tree above the cut).  No height of
scipy.cluster.hierarchy.linkage(X, 'average', 'cosine') lies within 1e-4 of t (asserted): an fp32 dot product of two means at D <= 512 is
off by at most about D * 6e-8 = 3e-5, so an fp32 implementation must give the same partition outright.  The seeds below were picked so
that the condition holds.  sklearn refuses a single sample, so the one-row case stores the only possible answer.
sklearn and scipy are needed here only, not by the tests."""
import os

import numpy as np
import sklearn
from scipy.cluster.hierarchy import linkage
from sklearn.cluster import AgglomerativeClustering

GAP = 1e-4
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "agglomerative.npz")


def canonical(labels):
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32)


def nested_blobs(rng, top, sub, per, D, subspread, spread):
    """`top` centres, `sub` sub-centres around each, `per` rows around each of those: merges at several levels"""
    c = rng.standard_normal((top, D))
    c = (c[:, None, :] + subspread * rng.standard_normal((top, sub, D))).reshape(-1, D)
    X = (c[:, None, :] + spread * rng.standard_normal((len(c), per, D))).reshape(-1, D).astype(np.float32)
    return X[rng.permutation(len(X))]


def cases():
    out = {}
    rng = np.random.default_rng(20261018)
    X = nested_blobs(rng, 5, 4, 14, 16, 0.45, 0.18)
    X = np.concatenate([X, X[7:8], X[7:8], 3 * rng.standard_normal((20, 16)).astype(np.float32)])     # two exact duplicates of row 7
    out["blobs16_t024"] = (X, 0.24)
    out["blobs16_t010"] = (X, 0.1)
    rng = np.random.default_rng(20261019)
    X = np.concatenate([nested_blobs(rng, 1, 6, 40, 128, 0.5, 0.6), -nested_blobs(rng, 1, 1, 4, 128, 0.5, 0.1)])
    out["blobs128_t06"] = (X, 0.6)
    out["noise_120x32"] = (rng.standard_normal((120, 32)).astype(np.float32), 0.24)                   # near-orthogonal: all single
    a = rng.standard_normal(24)
    out["two_rows_merge"] = (np.stack([a, 2 * a + 0.3 * rng.standard_normal(24)]).astype(np.float32), 0.24)
    out["two_rows_apart"] = (rng.standard_normal((2, 24)).astype(np.float32), 0.24)
    out["one_row"] = (rng.standard_normal((1, 24)).astype(np.float32), 0.24)
    return out


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    data = {}
    for name, (X, t) in cases().items():
        if len(X) > 1:
            h = linkage(X.astype(np.float64), 'average', 'cosine')[:, 2]
            assert not np.any(np.abs(h - t) < GAP), (name, "a merge height within 1e-4 of t", float(np.abs(h - t).min()))
            m = AgglomerativeClustering(n_clusters=None, linkage='average', distance_threshold=t, metric='cosine').fit(X)
            labels, gap = canonical(m.labels_), float(np.abs(h - t).min())
        else:
            labels, gap = np.zeros(1, np.int32), np.inf
        data[name + "__X"] = X
        data[name + "__t"] = np.float64(t)
        data[name + "__labels"] = labels
        print("{:16s} N={:4d} D={:3d} t={}: {} clusters, largest {}, nearest height {:.2e} from t".format(
            name, len(X), X.shape[1], t, labels.max() + 1, np.bincount(labels).max(), gap))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
