"""Generates tests/golden/optics.npz: sklearn 1.7.2's OPTICS(min_samples, max_eps, metric='cosine', cluster_method='dbscan') on small
fixtures, next to the float64 walk of tests/optics_cpu_kernels.py.

    python tests/golden/make_goldens_optics.py

Every case stores X (float32), max_eps, min_samples; sklearn's labels_ and core_distances_ (run on the float64 copy of X, so that
its distances are the float64 ones of rule 1); optics_fp64's ordering, reachability and predecessor; and, for the host cut,
sklearn's own reachability_ / ordering_ with sklearn.cluster.cluster_optics_dbscan of them at three eps values.

sklearn's ordering_ is NOT a target of the device tests: on the structural ties of OPTICS (every row relaxed at its predecessor's core
distance) its order is decided in the 15th decimal, and after such a flip its reachabilities differ too.  The target is optics_fp64's
walk, whose ties go to the lowest row.

The exact-order cases ("exact_*") must be decidable in fp32: the generator searches seeds from a fixed start and takes the first whose
float64 walk has  gap >= 4 (Dp + 8) 2^-24  (optics_fp64(want_gap=True): the distance of any pair from max_eps, the spacing of every row's
first min_samples + 1 sorted distances, and at every pick / relax comparison the margin between the two values compared unless they
are exactly equal).  (Dp + 8) 2^-24 bounds |d32 - d64| on unit rows; the factor 4 leaves twice the two-sided error.  The cases with
min_samples = 4 must also hold a border row with a finite reachability and a border row that rule 5's s < b test turns into noise.
sklearn is needed here only, not by the tests."""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import OPTICS, cluster_optics_dbscan

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from optics_cpu_kernels import fp64_distances, optics_fp64  # noqa: E402

OUT = os.path.join(HERE, "optics.npz")
SEED0 = 20261020

# name -> (N, D, blobs, sigma, min_samples, max_eps, border rows required)
EXACT = {
    "exact_d16_a": (120, 16, 5, 0.5, 4, 0.10, True),
    "exact_d16_b": (120, 16, 5, 0.6, 4, 0.12, True),
    "exact_d8": (150, 8, 6, 0.35, 4, 0.03, True),
    "exact_d33_ms2": (200, 33, 6, 0.4, 2, 0.14, False),                    # Dp = 40: the zero-padded columns
}


def blobs(seed, N, D, K, sigma):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((K, D))
    return (cen[rng.integers(0, K, N)] + sigma * rng.standard_normal((N, D))).astype(np.float32)


def border_kinds(X, o, max_eps):
    """(border rows with a finite reachability, non-core rows with a core neighbour that rule 5 leaves noise)"""
    d = fp64_distances(X)
    core = o["is_core"]
    has_core_nb = ((d <= max_eps) & core[None, :]).any(axis=1) & ~core
    return int((has_core_nb & np.isfinite(o["reachability"])).sum()), int((has_core_nb & (o["labels"] < 0)).sum())


def exact_case(name):
    N, D, K, sigma, ms, eps, need_border = EXACT[name]
    need = 4 * ((D + 7) // 8 * 8 + 8) * 2.0 ** -24
    for seed in range(SEED0, SEED0 + 400):
        X = blobs(seed, N, D, K, sigma)
        o = optics_fp64(X, eps, ms, want_gap=True)
        if o["gap"] < need:
            continue
        fin, noise = border_kinds(X, o, eps)
        if need_border and (fin < 1 or noise < 1):
            continue
        print("{:14s} seed {} gap {:.3g} (needs {:.3g}), {} border rows reached, {} left noise by s < b".format(
            name, seed, o["gap"], need, fin, noise))
        return X, eps, ms, o
    raise SystemExit("no seed passes for " + name)


def plain_cases():
    """no gap condition: labels, core distances and the host cut only"""
    out = {}
    out["plain_d24_ms3"] = (blobs(SEED0 + 1000, 300, 24, 6, 0.55), 0.20, 3)
    out["plain_d128_ms5"] = (blobs(SEED0 + 1001, 260, 128, 5, 0.5), 0.20, 5)
    X = blobs(SEED0 + 1002, 200, 12, 4, 0.4)
    out["plain_noise"] = (np.random.default_rng(SEED0 + 1003).standard_normal((90, 32)).astype(np.float32), 0.2, 3)
    out["plain_d12_ms2"] = (X, 0.08, 2)
    return out


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    todo = []
    for name in EXACT:
        X, eps, ms, o = exact_case(name)
        todo.append((name, X, eps, ms, o))
    for name, (X, eps, ms) in plain_cases().items():
        todo.append((name, X, eps, ms, optics_fp64(X, eps, ms)))
    data = {}
    for name, X, eps, ms, o in todo:
        d = fp64_distances(X)
        off = ~np.eye(len(X), dtype=bool)
        assert np.abs(d[off] - eps).min() > 1e-9, (name, "a pair at max_eps")
        m = OPTICS(min_samples=ms, max_eps=eps, metric='cosine', cluster_method='dbscan').fit(X.astype(np.float64))
        assert np.array_equal(m.labels_, o["labels"]), (name, "closed-form labels differ from sklearn's")
        fin = np.isfinite(m.core_distances_)
        assert np.array_equal(fin, o["is_core"]) and np.abs(m.core_distances_[fin] - o["core_distances"][fin]).max(initial=0.0) <= 1e-12, name
        cut_eps = np.array([0.45, 0.7, 0.9]) * eps
        cuts = np.stack([cluster_optics_dbscan(reachability=m.reachability_, core_distances=m.core_distances_,
                                               ordering=m.ordering_, eps=e) for e in cut_eps])
        data[name + "__X"] = X
        data[name + "__max_eps"] = np.float64(eps)
        data[name + "__min_samples"] = np.int64(ms)
        data[name + "__sk_labels"] = m.labels_.astype(np.int32)
        data[name + "__sk_core_distances"] = m.core_distances_.astype(np.float64)
        data[name + "__sk_reachability"] = m.reachability_.astype(np.float64)
        data[name + "__sk_ordering"] = m.ordering_.astype(np.int32)
        data[name + "__cut_eps"] = cut_eps
        data[name + "__cut_labels"] = cuts.astype(np.int32)
        data[name + "__ordering"] = o["ordering"]
        data[name + "__reachability"] = o["reachability"]
        data[name + "__predecessor"] = o["predecessor"]
        same = np.array_equal(m.ordering_, o["ordering"])
        print("{:14s} N={:4d} D={:3d} max_eps={} ms={}: {} clusters, {} noise, {} core; sklearn's ordering {} the lowest-row walk".format(
            name, len(X), X.shape[1], eps, ms, o["n_clusters"], int((o["labels"] < 0).sum()), int(o["is_core"].sum()),
            "equals" if same else "differs from"))
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
