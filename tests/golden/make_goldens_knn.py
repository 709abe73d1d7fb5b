"""Writes tests/golden/knn.npz: what sklearn 1.7.2's KNeighborsClassifier / NearestNeighbors return on one small seeded data set.

    python tests/golden/make_goldens_knn.py

Data: 7 Gaussian classes (sigma 1.1) around unit-normal centres in 24 dimensions, 600 gallery rows, 96 queries of which 4 are copies
of gallery rows (the zero-distance rule of weights='distance'); the labels are NOT 0 .. C-1.  One data set per metric (another seed).

Per metric in ('cosine', 'euclidean'), weights in ('uniform', 'distance') and k in (1, 5, 20, 88):
    <metric>/<weights>/<k>/predict, /proba, /score      sklearn's predict, predict_proba, score on the float64 rows
    <metric>/<weights>/<k>/skip                         queries whose two best class probabilities differ by less than 1e-4 in the
                                                        float64 oracle (tests/knn_cpu_kernels.py vote64): float32 distances may decide
                                                        them either way.  'uniform' skips nobody: its scores are whole numbers.
    <metric>/loo_idx                                    NearestNeighbors.kneighbors(X=None, n_neighbors=5) on the gallery

So that sklearn's arbitrary order among ties cannot decide a case, asserted here in float64 — a violating seed is changed, rows are never
dropped:
  * every query has a gap of at least 1e-5 between its k-th and (k+1)-th distance, for every k above (and the leave-one-out rows at 5);
  * at most 2 % of the queries of a case are skipped;
  * the float64 oracle agrees with sklearn on every query that is not skipped.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.neighbors import KNeighborsClassifier, NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from knn_cpu_kernels import DISTANCE, UNIFORM, distances64, search64, vote64      # noqa: E402

assert sklearn.__version__ == "1.7.2", sklearn.__version__
SEEDS = {"cosine": 268, "euclidean": 86}      # the widest smallest gap among seeds 1 .. 399
KS = (1, 5, 20, 88)
LABEL_VALUES = np.array([3, 7, 40, 41, 99, 250, 1001], np.int64)
N_CLASSES, D, NG, NQ, N_COPIES, SIGMA = 7, 24, 600, 96, 4, 1.1
MIN_GAP, SCORE_GAP, MAX_SKIP = 1e-5, 1e-4, 0.02


def make(seed):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((N_CLASSES, D))
    yg, yq = rng.integers(0, N_CLASSES, NG), rng.integers(0, N_CLASSES, NQ)
    g = (cen[yg] + SIGMA * rng.standard_normal((NG, D))).astype(np.float32)
    q = (cen[yq] + SIGMA * rng.standard_normal((NQ, D))).astype(np.float32)
    rows = rng.choice(NG, N_COPIES, replace=False)
    q[:N_COPIES] = g[rows]
    yq[:N_COPIES] = yg[rows]
    return g, LABEL_VALUES[yg], q, LABEL_VALUES[yq]


def assert_gaps(d, ks, what):
    s = np.sort(d, axis=1)
    for k in ks:
        gap = (s[:, k] - s[:, k - 1]).min()
        assert gap >= MIN_GAP, "%s: gap %.3g between ranks %d | %d" % (what, gap, k, k + 1)
        print("  %s: smallest gap at k = %d: %.3g" % (what, k, gap))


out = {}
for metric, seed in SEEDS.items():
    g, yg, q, yq = make(seed)
    out.update({metric + "/gallery": g, metric + "/gallery_labels": yg, metric + "/queries": q, metric + "/query_labels": yq})
    g64, q64 = g.astype(np.float64), q.astype(np.float64)
    assert_gaps(distances64(q, g, metric), KS, metric)
    loo = distances64(g, None, metric)
    np.fill_diagonal(loo, np.inf)
    assert_gaps(loo, (5,), metric + " leave-one-out")
    nn = NearestNeighbors(n_neighbors=5, metric=metric, algorithm="brute").fit(g64)
    loo_idx = nn.kneighbors(None, return_distance=False)
    assert np.array_equal(loo_idx, search64(g, None, 5, metric)[0])
    out[metric + "/loo_idx"] = loo_idx.astype(np.int32)
    classes, dense = np.unique(yg, return_inverse=True)
    for weights, mode in (("uniform", UNIFORM), ("distance", DISTANCE)):
        for k in KS:
            clf = KNeighborsClassifier(n_neighbors=k, weights=weights, metric=metric, algorithm="brute").fit(g64, yg)
            pred, proba, score = clf.predict(q64), clf.predict_proba(q64), clf.score(q64, yq)
            idx, dist = search64(q, g, k, metric)
            p64, top, _, _ = vote64(idx, dist, dense, len(classes), mode, 1.0, 1)
            two = np.sort(p64, axis=1)[:, ::-1][:, :2]
            skip = np.zeros(NQ, bool) if weights == "uniform" else (two[:, 0] - two[:, 1]) < SCORE_GAP
            assert skip.mean() <= MAX_SKIP, (metric, weights, k, int(skip.sum()))
            assert np.array_equal(classes[top[:, 0]][~skip], pred[~skip]), (metric, weights, k)
            key = "%s/%s/%d/" % (metric, weights, k)
            out[key + "predict"], out[key + "proba"], out[key + "score"], out[key + "skip"] = pred, proba, np.float64(score), skip
            print("  %s: sklearn score %.4f, skipped %d, max |proba - oracle| %.3g" % (key, score, skip.sum(), np.abs(proba - p64).max()))

path = os.path.join(HERE, "knn.npz")
np.savez_compressed(path, **out)
print("wrote knn.npz", os.path.getsize(path), "bytes")
