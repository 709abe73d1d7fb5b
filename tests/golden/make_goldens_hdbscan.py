"""Generates tests/golden/hdbscan.npz: sklearn 1.7.2's HDBSCAN(metric='cosine') on small fixtures (<= 500 rows, D = 32).

    python tests/golden/make_goldens_hdbscan.py

sklearn's labels depend on the order of the rows: mutual reachability ties structurally (w = core(i) for several j), and Prim's walk
with an unstable argsort decides which side such a row falls on.  So every case is run under PERMS row permutations and stores, next to
the labels and probabilities of the given order, a per-row `stable` mask: the rows whose cluster and probability are the same under
every permutation (clusters matched by majority).  Asserted here: at most 2 % of the rows fall outside the mask, none at min_samples = 2; the masked labels survive a
symmetric perturbation of the distance matrix by +-4e-6 (four trials: the fp32 error of a device score is well inside that); no MST
weight lies within 1e-4 of a stored dbscan_clustering cut.  sklearn is needed here only, not by the tests."""
import os

import numpy as np
import sklearn
from sklearn.cluster import HDBSCAN
from sklearn.metrics import pairwise_distances

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hdbscan.npz")
PERMS = 12
D = 32


def unit(X):
    return (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)


def clustered(rng, K, per, spread, n_noise):
    cen = rng.standard_normal((K, D))
    rows = [c + spread * rng.uniform(0.6, 1.4) * rng.standard_normal((per, D)) for c in cen]
    rows.append(rng.standard_normal((n_noise, D)))                  # uniform on the sphere once normalised
    X = np.concatenate(rows)
    return unit(X[rng.permutation(len(X))])


def by_smallest_row(labels):
    out, seen = np.full(len(labels), -1, np.int32), {}
    for i, l in enumerate(np.asarray(labels).tolist()):
        if l >= 0:
            out[i] = seen.setdefault(l, len(seen))
    return out


def matched(labels, ref):
    """labels renamed so that every cluster carries the name of the cluster of `ref` most of its rows are in"""
    out = np.full(len(labels), -1, np.int64)
    for l in set(labels.tolist()) - {-1}:
        rows = labels == l
        names, counts = np.unique(ref[rows], return_counts=True)
        out[rows] = names[np.argmax(counts)] if names[np.argmax(counts)] >= 0 else -2
    return out


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return (np.array_equal(a < 0, b < 0) and len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs)))


def cases():
    rng = np.random.default_rng(20261021)
    A = clustered(rng, 6, 70, 0.22, 65)                              # 485 rows
    B = clustered(rng, 5, 60, 0.2, 40)
    B[17] = B[3]                                                     # two exact duplicate rows
    C = unit(rng.standard_normal((1, D)) + 0.25 * rng.standard_normal((200, D)))      # one blob: a single cluster
    # tight blobs, few noise rows: with min_cluster_size = 3 one tie can move a cluster's deepest split, and with it the probabilities of
    # all its rows; most data sets of the kind above lose a whole cluster from the mask
    T = clustered(np.random.default_rng(100), 6, 50, 0.1, 8)
    kw = dict(method='eom', eps=0.0, single=False, cuts=())
    out = {}
    for name, X, mcs, ms, extra in [
            ("a_mcs5", A, 5, None, {}), ("a_mcs5_ms2", A, 5, 2, dict(cuts=(0.15, 0.3))), ("a_mcs10_ms3", A, 10, 3, {}),
            ("t_mcs3_ms3", T, 3, 3, {}), ("a_leaf_mcs5_ms2", A, 5, 2, dict(method='leaf')), ("a_leaf_mcs8_ms4", A, 8, 4, dict(method='leaf')),
            ("a_leaf_eps_mcs5_ms2", A, 5, 2, dict(method='leaf', eps=0.25)), ("dup_mcs5_ms2", B, 5, 2, {}), ("one_single_mcs5_ms2", C, 5, 2, dict(single=True))]:
        out[name] = (X, mcs, ms, dict(kw, **extra))
    return out


def fit(X64, mcs, ms, o, precomputed=False):
    return HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric='precomputed' if precomputed else 'cosine', cluster_selection_method=o["method"],
                   cluster_selection_epsilon=float(o["eps"]), allow_single_cluster=o["single"], copy=True).fit(X64)


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    rng = np.random.default_rng(7)
    data = {}
    for name, (X, mcs, ms, o) in cases().items():
        N = len(X)
        X64 = X.astype(np.float64)
        ref = fit(X64, mcs, ms, o)
        lab0, p0 = by_smallest_row(ref.labels_), ref.probabilities_
        stable = np.ones(N, bool)
        for _ in range(PERMS):
            perm = rng.permutation(N)
            m = fit(X64[perm], mcs, ms, o)
            lab, p = np.empty(N, np.int64), np.empty(N)
            lab[perm], p[perm] = m.labels_, m.probabilities_
            stable &= (matched(lab, lab0) == lab0) & (np.abs(p - p0) <= 1e-9)
        n_out = int((~stable).sum())
        assert n_out <= 0.02 * N, (name, n_out)
        eff_ms = mcs if ms is None else ms
        assert eff_ms != 2 or n_out == 0, (name, n_out)
        Dm = pairwise_distances(X64, metric='cosine')
        for _ in range(4):
            E = np.triu(rng.uniform(-4e-6, 4e-6, (N, N)), 1)
            Dp = np.clip(Dm + E + E.T, 0.0, 2.0)
            np.fill_diagonal(Dp, 0.0)
            m = fit(Dp, mcs, ms, o, precomputed=True)
            assert same_partition(by_smallest_row(m.labels_)[stable], lab0[stable]), (name, "labels move under a 4e-6 perturbation")
        mstw = np.asarray(ref._single_linkage_tree_["value"])
        h_min = float(mstw[mstw > 0].min())
        data[name + "__X"] = X
        data[name + "__params"] = np.asarray([mcs, -1 if ms is None else ms, o["method"] == 'leaf', o["single"]], np.int64)
        data[name + "__eps"] = np.float64(o["eps"])
        data[name + "__labels"] = ref.labels_.astype(np.int32)
        data[name + "__prob"] = ref.probabilities_.astype(np.float64)
        data[name + "__stable"] = stable
        data[name + "__cuts"] = np.asarray(o["cuts"], np.float64)
        for c, cut in enumerate(o["cuts"]):
            assert np.abs(mstw - cut).min() > 1e-4, (name, cut)
            data[name + "__cut{}".format(c)] = ref.dbscan_clustering(cut, mcs).astype(np.int32)
        print("{:20s} N={:4d} mcs={} ms={} {}: {} clusters, {} noise, {} rows outside the mask, smallest MST weight {:.3g}".format(
            name, N, mcs, ms, o, int(ref.labels_.max()) + 1, int((ref.labels_ < 0).sum()), n_out, h_min))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
