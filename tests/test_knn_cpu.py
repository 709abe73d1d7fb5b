"""CPU: the host logic of neighbors.py (NearestNeighbors, KNeighborsClassifier), evaluate.knn_classify / retrieval_metrics and the
VAL.KNN_K hook of k_nearest_embeddings, driven with the NumPy provider (tests/knn_cpu_kernels.py) against sklearn 1.7.2's results
(tests/golden/knn.npz, written by tests/golden/make_goldens_knn.py) and a float64 oracle.  The same cases on the HIP kernels:
tests/test_knn_gpu.py."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ns = types.SimpleNamespace
KS = (1, 5, 20, 88)
GOLDEN_CASES = [(m, w, k) for m in ("cosine", "euclidean") for w in ("uniform", "distance") for k in KS]


def proba_bound_fp32(k):
    """|float32 vote on float32 distances - sklearn's float64 proba|: a distance rounded to float32 and the division 1 / d cost 2^-24
    relative each, the k additions of a class score and of the total another k 2^-24, the final division one more: (2 k + 8) 2^-24
    with room for the second-order terms.  (sklearn's euclidean distance of a copied row is ~1e-7, not 0: its weight 1e7 and the
    rule's (d == 0) give probabilities that differ by sum(1 / d_j) / 1e7, below this bound at every k here.)"""
    return (2 * k + 8) * 2.0 ** -24


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "knn.npz")))


@pytest.mark.parametrize("metric,weights,k", GOLDEN_CASES)
def test_classifier_vs_sklearn(golden, metric, weights, k):
    from video_similarity_search_amd.neighbors import KNeighborsClassifier
    from knn_cpu_kernels import NumpyKnnKernels
    g = golden
    key = "%s/%s/%d/" % (metric, weights, k)
    clf = KNeighborsClassifier(n_neighbors=k, weights=weights, metric=metric, kernels=NumpyKnnKernels())
    assert clf.fit(g[metric + "/gallery"], g[metric + "/gallery_labels"]) is clf
    assert np.array_equal(clf.classes_, np.unique(g[metric + "/gallery_labels"])) and clf.n_samples_fit_ == 600
    skip = g[key + "skip"]
    assert skip.mean() <= 0.02
    pred = clf.predict(g[metric + "/queries"])
    assert isinstance(pred, np.ndarray) and pred.dtype == g[key + "predict"].dtype
    assert np.array_equal(pred[~skip], g[key + "predict"][~skip])
    proba = clf.predict_proba(g[metric + "/queries"])
    assert torch.is_tensor(proba) and proba.dtype == torch.float32 and tuple(proba.shape) == (96, 7)
    if weights == "uniform":
        assert np.array_equal(proba.numpy(), g[key + "proba"].astype(np.float32))           # multiples of 1 / k: outright
    else:
        err = np.abs(proba.numpy().astype(np.float64) - g[key + "proba"]).max()
        print("max |proba - sklearn| = %.3g (bound %.3g)" % (err, proba_bound_fp32(k)))
        assert err <= proba_bound_fp32(k)
    score = clf.score(g[metric + "/queries"], g[metric + "/query_labels"])
    assert abs(score - float(g[key + "score"])) <= skip.sum() / 96.0 + 1e-12


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_leave_one_out_kneighbors(golden, metric):
    from video_similarity_search_amd.neighbors import KNeighborsClassifier, NearestNeighbors
    from knn_cpu_kernels import NumpyKnnKernels
    X, y = golden[metric + "/gallery"], golden[metric + "/gallery_labels"]
    nn = NearestNeighbors(n_neighbors=5, metric=metric, kernels=NumpyKnnKernels()).fit(X)
    dist, idx = nn.kneighbors()
    assert np.array_equal(idx.numpy(), golden[metric + "/loo_idx"])
    assert not (idx.numpy() == np.arange(600)[:, None]).any()
    assert (np.diff(dist.numpy(), axis=1) >= 0).all()
    assert torch.equal(nn.kneighbors(None, return_distance=False), idx)
    assert tuple(nn.kneighbors(X[:7], n_neighbors=3)[1].shape) == (7, 3)
    # the classifier's leave-one-out form votes on those lists
    clf = KNeighborsClassifier(n_neighbors=5, metric=metric, kernels=NumpyKnnKernels()).fit(X, y)
    classes, dense = np.unique(y, return_inverse=True)
    votes = dense[golden[metric + "/loo_idx"]]
    want = classes[np.array([np.bincount(v, minlength=len(classes)).argmax() for v in votes])]
    assert np.array_equal(clf.predict(), want)


def test_softmax_weights_and_tensor_labels(golden):
    """weights='softmax' is the monitor's exp(sim / T) vote: against the float64 oracle; labels given as a tensor"""
    from video_similarity_search_amd.neighbors import KNeighborsClassifier
    from knn_cpu_kernels import NumpyKnnKernels, SOFTMAX, search64, vote64
    X, y, Q = golden["cosine/gallery"], golden["cosine/gallery_labels"], golden["cosine/queries"]
    clf = KNeighborsClassifier(n_neighbors=20, weights="softmax", temperature=0.07, kernels=NumpyKnnKernels()).fit(X, torch.from_numpy(y))
    classes, dense = np.unique(y, return_inverse=True)
    assert np.array_equal(clf.classes_, classes)
    idx, dist = search64(Q, X, 20, "cosine")
    p64, top, _, _ = vote64(idx, dist, dense, 7, SOFTMAX, 0.07, 1)
    # exp((d0 - d) / T) with d0 - d down to -0.5 / 0.07: an absolute error 2^-24 |d| of a float32 distance becomes a relative error
    # 2^-24 / 0.07 of the weight, 2^-23 more for the product and the exp; sums as in proba_bound_fp32 -> (2 / 0.07 + 2 k + 8) 2^-24
    assert np.abs(clf.predict_proba(Q).numpy() - p64).max() <= (2 / 0.07 + 48) * 2.0 ** -24
    two = np.sort(p64, axis=1)[:, ::-1]
    sure = two[:, 0] - two[:, 1] >= 1e-4
    assert sure.mean() >= 0.98 and np.array_equal(clf.predict(Q)[sure], classes[top[:, 0]][sure])


def test_vote_restatement_rules():
    """the float32 restatement against the float64 oracle on the shared hand-made tables, and the rules by hand on a tiny one"""
    from knn_cases import VOTE_CASES, vote_case
    from knn_cpu_kernels import DISTANCE, SOFTMAX, UNIFORM, vote32, vote64
    idx = np.array([[0, 1, -1, 2, 3], [-1, -1, 9, -1, -1], [4, 0, 1, 2, 3]], np.int32)
    dist = np.array([[0.0, 0.0, 0.0, 0.5, 1.0], [0, 0, 0, 0, 0], [0.25, 0.5, 0.5, 1.0, 2.0]], np.float32)
    g_labels = np.array([1, 0, 1, 2, -1], np.int64)                    # row 4: noise; C = 2 leaves row 3's class 2 out too
    proba, pred, score, s = vote32(idx, dist, g_labels, 2, DISTANCE, 1.0, 3)
    assert np.array_equal(s, [[1, 1], [0, 0], [2, 3]])                  # row 0: zero rule, the 0.5 gets no weight; row 2: 1 / d
    assert np.array_equal(pred, [[0, 1, -1], [-1, -1, -1], [1, 0, -1]])  # the tie goes to the lower class; nothing past C
    assert np.array_equal(score, [[1, 1, 0], [0, 0, 0], [3, 2, 0]])
    assert np.array_equal(proba[1], [0, 0]) and np.allclose(proba[2], [0.4, 0.6])
    proba, pred, _, s = vote32(idx, None, g_labels, 3, UNIFORM, 1.0, 1)
    assert np.array_equal(s, [[1, 2, 1], [0, 0, 0], [1, 2, 1]]) and np.array_equal(pred[:, 0], [1, -1, 1])
    _, _, _, s = vote32(idx, dist, g_labels, 2, SOFTMAX, 0.5, 1)        # row 2 opens with the noise row: d_first is rank 1's 0.5
    assert np.allclose(s[2], [1.0, 1.0 + np.exp(-1.0)])
    for (k, Nq, C, n_top) in VOTE_CASES:
        tab = vote_case(k, Nq, C)
        for mode in (UNIFORM, DISTANCE, SOFTMAX):
            p32, pred32, _, s32 = vote32(*tab, C, mode, 0.07, n_top)
            p64, pred64, _, s64 = vote64(*tab, C, mode, 0.07, n_top)
            fin = np.isfinite(s64).all(1)
            assert np.abs(p32[fin] - p64[fin]).max() <= (2 * k + 8 + 2 / 0.07) * 2.0 ** -24
            assert ((pred32 >= 0) == (pred64 >= 0)).all()


def oracle_ranked(idx, q_labels, g_labels, n_rel, ks):
    """precision@K, recall@K, AP@K, RR per query from cumulative sums in float64 — written independently of knn_cpu_kernels.ranked64"""
    ok = (idx >= 0) & (idx < len(g_labels))
    h = ok & (g_labels[np.where(ok, idx, 0)] == q_labels[:, None])
    c = np.cumsum(h, axis=1).astype(np.float64)
    terms = np.where(h, c / np.arange(1, idx.shape[1] + 1), 0.0)
    pq = np.zeros((idx.shape[0], len(ks), 3))
    nr = n_rel.astype(np.float64)
    for a, K in enumerate(ks):
        pq[:, a, 0] = c[:, K - 1] / K
        pq[:, a, 1] = np.where(nr > 0, c[:, K - 1] / np.maximum(nr, 1), 0.0)
        pq[:, a, 2] = np.where(nr > 0, terms[:, :K].sum(1) / np.maximum(np.minimum(nr, K), 1), 0.0)
    rr = np.where(h.any(1), 1.0 / (h.argmax(1) + 1), 0.0)
    return pq, rr


def test_ranked_restatement():
    from knn_cases import RANKED_CASES, ranked_case
    from knn_cpu_kernels import ranked64
    for (k, Nq, ks) in RANKED_CASES:
        idx, ql, gl, n_rel = ranked_case(k, Nq, ks)
        pq, rr, rec = ranked64(idx, ql, gl, n_rel, ks)
        opq, orr = oracle_ranked(idx, ql, gl, n_rel, ks)
        assert np.allclose(pq, opq, rtol=1e-12, atol=0) and np.allclose(rr, orr, rtol=1e-12, atol=0)
        rel = n_rel > 0
        assert rec[-1] == rel.sum() and np.isclose(rec[-2], orr.mean(), rtol=1e-12)
        for a in range(len(ks)):
            assert np.isclose(rec[3 * a], opq[:, a, 0].mean(), rtol=1e-12)
            if rel.any():
                assert np.allclose(rec[3 * a + 1:3 * a + 3], opq[rel, a, 1:].mean(0), rtol=1e-12)
    # by hand: hits at ranks 1 and 3 of 4, three relevant rows
    pq, rr, _ = ranked64(np.array([[5, 0, 6, 1]]), np.array([1]), np.array([1, 1, 1, 0, 0, 0, 0]), np.array([3]), (1, 2, 4))
    assert np.allclose(pq[0], [[0, 0, 0], [0.5, 1 / 3, (1 / 2) / 2], [0.5, 2 / 3, (1 / 2 + 2 / 4) / 3]]) and rr[0] == 0.5


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_retrieval_metrics(golden, metric):
    """against the float64 oracle; the query labels are bent so that some queries have no relevant row and some fewer than K"""
    from video_similarity_search_amd.evaluate import retrieval_metrics
    from knn_cpu_kernels import NumpyKnnKernels, search64
    X, y, Q = golden[metric + "/gallery"], golden[metric + "/gallery_labels"].copy(), golden[metric + "/queries"]
    yq = golden[metric + "/query_labels"].copy()
    yq[5:9] = 123456                                                    # a label the gallery does not hold: n_rel = 0
    rare = np.flatnonzero(y == 1001)[3:]
    y[rare] = 3                                                         # class 1001 keeps three rows: n_rel = 3 < K for K = 5 ..
    assert (y == 1001).sum() == 3 and (yq == 1001).any()
    ks = (1, 5, 10, 20, 50)
    K = NumpyKnnKernels()
    out = retrieval_metrics(Q, yq, X, y, ks=ks, dist_metric=metric, kernels=K)
    assert K.reads == 1 and [c[0] for c in K.calls] == ["search", "ranked"] and K.calls[0][1] == 50
    idx, _ = search64(Q, X, 50, metric)
    n_rel = np.array([(y == l).sum() for l in yq])
    assert (n_rel == 0).sum() == 4 and ((n_rel > 0) & (n_rel < 5)).any()
    pq, rr = oracle_ranked(idx, yq, y, n_rel, ks)
    rel = n_rel > 0
    assert out["n_with_relevant"] == rel.sum() == 92 and np.isclose(out["mrr"], rr.mean(), rtol=1e-12)
    assert set(out) == {"precision", "recall", "map", "mrr", "n_with_relevant"}
    for a, k in enumerate(ks):
        assert np.isclose(out["precision"][k], pq[:, a, 0].mean(), rtol=1e-12)
        assert np.isclose(out["recall"][k], pq[rel, a, 1].mean(), rtol=1e-12)
        assert np.isclose(out["map"][k], pq[rel, a, 2].mean(), rtol=1e-12)
    # leave-one-out: a row is not its own neighbour and not among its own relevant rows
    loo = retrieval_metrics(X, y, ks=(1, 5), dist_metric=metric, kernels=NumpyKnnKernels())
    idx, _ = search64(X, None, 5, metric)
    pq, rr = oracle_ranked(idx, y, y, np.array([(y == l).sum() - 1 for l in y]), (1, 5))
    assert np.isclose(loo["map"][5], pq[:, 1, 2].mean(), rtol=1e-12) and np.isclose(loo["mrr"], rr.mean(), rtol=1e-12)
    assert loo["n_with_relevant"] == 600


@pytest.mark.parametrize("weights", ["uniform", "distance", "softmax"])
def test_knn_classify(golden, weights):
    from video_similarity_search_amd.evaluate import knn_classify
    from knn_cpu_kernels import NumpyKnnKernels, search64, vote32
    from video_similarity_search_amd.neighbors import WEIGHTS
    X, Q = golden["cosine/gallery"], golden["cosine/queries"]
    _, y = np.unique(golden["cosine/gallery_labels"], return_inverse=True)
    _, yq = np.unique(golden["cosine/query_labels"], return_inverse=True)
    y = y.copy()
    y[::50] = -1                                                        # noise pseudo-labels never vote
    K = NumpyKnnKernels()
    out = knn_classify(Q, yq, X, y, k=20, weights=weights, top_n=(1, 3, 5), num_classes=7, kernels=K)
    assert K.reads == 1 and [c[0] for c in K.calls] == ["search", "vote"]
    idx, dist = search64(Q, X, 20, "cosine")
    _, pred, score, _ = vote32(idx, dist.astype(np.float32), y, 7, WEIGHTS[weights], 0.07, 5)
    match = (pred == yq[:, None]) & (score > 0)
    assert set(out) == {"top1", "top3", "top5", "mean_class_acc", "n_queries"} and out["n_queries"] == 96
    for n in (1, 3, 5):
        assert out["top%d" % n] == match[:, :n].any(1).mean()
    per_class = [match[yq == c, 0].mean() for c in range(7) if (yq == c).any()]
    assert np.isclose(out["mean_class_acc"], np.mean(per_class), rtol=1e-12)
    assert 0.9 < out["top1"] <= out["top3"] <= out["top5"] <= 1.0
    # leave-one-out on one set, the class count taken from the labels
    K = NumpyKnnKernels()
    loo = knn_classify(X, np.maximum(y, 0), k=5, weights=weights, kernels=K)
    assert K.calls[0] == ("search", 5, "cosine") and set(loo) == {"top1", "top5", "mean_class_acc", "n_queries"} and loo["n_queries"] == 600


def test_raises(golden):
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.evaluate import knn_classify, retrieval_metrics
    from video_similarity_search_amd.neighbors import KNeighborsClassifier, NearestNeighbors
    from knn_cpu_kernels import NumpyKnnKernels
    X, y = golden["cosine/gallery"], golden["cosine/gallery_labels"]
    K = NumpyKnnKernels()
    for kw, exc, pat in [(dict(weights=lambda d: d), NotImplementedError, "callable weights"),
                         (dict(p=1), NotImplementedError, "p=1"),
                         (dict(algorithm="kd_tree"), NotImplementedError, "algorithm='kd_tree'"),
                         (dict(algorithm="ball_tree"), NotImplementedError, "brute force"),
                         (dict(metric="manhattan"), NotImplementedError, "metric='manhattan'"),
                         (dict(metric="precomputed"), NotImplementedError, "precomputed"),
                         (dict(metric=lambda a, b: 0.0), NotImplementedError, "only 'cosine' and 'euclidean'"),
                         (dict(n_neighbors=89), ValueError, "beyond the 88"),
                         (dict(n_neighbors=0), ValueError, "Expected n_neighbors > 0"),
                         (dict(weights="gaussian"), ValueError, "weights must be"),
                         (dict(weights="softmax", temperature=0.0), ValueError, "temperature must be positive"),
                         (dict(metric="euclidean", precision="bf16"), ValueError, "unit rows"),
                         (dict(precision="fp16"), ValueError, "precision must be")]:
        with pytest.raises(exc, match=pat):
            KNeighborsClassifier(kernels=K, **kw).fit(X, y)
    with pytest.raises(NotImplementedError, match="radius"):
        NearestNeighbors(radius=1.0, kernels=K).fit(X)
    many = np.arange(4097)
    with pytest.raises(ValueError, match="4097 classes"):
        KNeighborsClassifier(kernels=K).fit(np.zeros((4097, 2), np.float32), many)
    with pytest.raises(ValueError, match="integer class labels"):
        KNeighborsClassifier(kernels=K).fit(X, y.astype(np.float32))
    with pytest.raises(ValueError, match="inconsistent numbers of samples"):
        KNeighborsClassifier(kernels=K).fit(X, y[:-1])
    clf = KNeighborsClassifier(kernels=K).fit(X, y)
    with pytest.raises(ValueError, match="beyond the 88"):
        clf.kneighbors(X[:3], n_neighbors=100)
    with pytest.raises(ValueError, match="n_neighbors <= n_samples_fit"):
        KNeighborsClassifier(n_neighbors=5, kernels=K).fit(X[:5], y[:5]).kneighbors()
    with pytest.raises(RuntimeError, match="not fitted"):
        KNeighborsClassifier(kernels=K).predict(X)
    with pytest.raises(ValueError, match="outside 1 .. 88"):
        knn_classify(X, y, k=89, num_classes=2000, kernels=K)
    with pytest.raises(ValueError, match="5000 classes"):
        knn_classify(X, y, k=5, num_classes=5000, kernels=K)
    with pytest.raises(ValueError, match="at most 8"):
        knn_classify(X, y, k=5, num_classes=2000, top_n=(1, 9), kernels=K)
    with pytest.raises(ValueError, match="weights must be"):
        knn_classify(X, y, k=5, weights="gaussian", kernels=K)
    with pytest.raises(ValueError, match="dist_metric"):
        knn_classify(X, y, k=5, dist_metric="manhattan", kernels=K)
    with pytest.raises(ValueError, match="beyond the 88"):
        retrieval_metrics(X, y, ks=(1, 100), kernels=K)
    with pytest.raises(ValueError, match="ascending"):
        retrieval_metrics(X, y, ks=(5, 1), kernels=K)
    with pytest.raises(ValueError, match="1 .. 8"):
        retrieval_metrics(X, y, ks=tuple(range(1, 10)), kernels=K)
    if not torch.cuda.is_available():                                   # the product path has no CPU fallback
        with pytest.raises(_lib.SlicError):
            KNeighborsClassifier().fit(X, y)
        with pytest.raises(_lib.SlicError):
            knn_classify(X, y, k=5, num_classes=2000)
        with pytest.raises(_lib.SlicError):
            retrieval_metrics(X, y, ks=(1, 5))


# ---- the VAL.KNN_K hook of k_nearest_embeddings -------------------------------------------------------------------------------
def embedding_loader(x, labels, batch):
    return [(torch.from_numpy(x[s:s + batch]), torch.from_numpy(labels[s:s + batch]), 0, torch.arange(s, min(s + batch, len(x))))
            for s in range(0, len(x), batch)]


def recording_provider():
    """the validation provider and the k-NN provider in one object, every kernel call noted in order"""
    from knn_cpu_kernels import NumpyKnnKernels
    from validate_cpu_kernels import NumpyValidationKernels

    class Both(NumpyValidationKernels, NumpyKnnKernels):
        def __init__(self):
            NumpyValidationKernels.__init__(self)
            NumpyKnnKernels.__init__(self)

        def topk(self, x, y, k, dist_metric):
            self.calls.append(("topk", int(k), dist_metric))
            return NumpyValidationKernels.topk(self, x, y, k, dist_metric)

        def label_hits(self, idx, q_labels, g_labels, top_ks):
            self.calls.append(("label_hits", tuple(idx.shape), tuple(top_ks)))
            return NumpyValidationKernels.label_hits(self, idx, q_labels, g_labels, top_ks)
    return Both()


@pytest.mark.parametrize("dm", ["cosine", "euclidean"])
def test_k_nearest_embeddings_hook(golden_dir, tmp_path, capsys, dm):
    from video_similarity_search_amd.evaluate import k_nearest_embeddings
    from knn_cpu_kernels import SOFTMAX, UNIFORM, search64, vote32
    g = dict(np.load(os.path.join(golden_dir, "validation.npz")))
    train_loader = embedding_loader(g["knn_train"], g["knn_train_labels"], 32)
    test_loader = embedding_loader(g["knn_test"], g["knn_test_labels"], 16)
    epoch = int(g["knn_epoch"])
    plain_out = 'Getting embeddings...\nComputing top1/5/10/20 Acc...\n' + str(g["knn_%s/print" % dm]) + '\n'

    def run(val, sub):
        cfg = ns(OUTPUT_PATH=str(tmp_path / sub), LOSS=ns(DIST_METRIC=dm), NUM_GPUS=1)
        if val is not None:
            cfg.VAL = val
        K = recording_provider()
        capsys.readouterr()
        acc = k_nearest_embeddings(None, torch.nn.Identity(), False, "cpu", train_loader, test_loader, None, None, cfg, plot=False,
                                   epoch=epoch, kernels=K)
        return acc, capsys.readouterr().out, K, os.path.join(str(tmp_path / sub), "tnet_checkpoints")

    # the key absent, the section there without the key, the key 0: the calls, prints, file and value of before
    for i, val in enumerate((None, ns(METRIC='global'), ns(KNN_K=0))):
        acc, out, K, d = run(val, "off%d" % i)
        assert K.calls == [("topk", 20, dm), ("label_hits", (40, 20), (1, 5, 10, 20))]
        assert isinstance(acc, np.ndarray) and acc.dtype == np.float64 and np.array_equal(acc, g["knn_%s/acc" % dm])
        assert out == plain_out
        assert os.listdir(d) == ["global_retrieval_acc.txt"]
        assert open(os.path.join(d, "global_retrieval_acc.txt")).read() == str(g["knn_%s/file" % dm])

    # KNN_K = 30: one search at 30, the four accuracies unchanged, one more line on the screen and in knn_acc.txt
    acc, out, K, d = run(ns(KNN_K=30), "on")
    assert K.calls == [("search", 30, dm), ("label_hits", (40, 20), (1, 5, 10, 20)), ("vote", 30, SOFTMAX, 5)]
    assert isinstance(acc, np.ndarray) and np.array_equal(acc, g["knn_%s/acc" % dm])
    idx, dist = search64(g["knn_test"], g["knn_train"], 30, dm)
    C = int(g["knn_train_labels"].max()) + 1
    _, pred, score, _ = vote32(idx, dist.astype(np.float32), g["knn_train_labels"], C, SOFTMAX, 0.07, 5)
    match = (pred == g["knn_test_labels"][:, None]) & (score > 0)
    top1, top5 = 100. * match[:, 0].mean(), 100. * match.any(1).mean()
    assert out == plain_out + 'kNN (k=30, softmax) Top1 Acc: {:.2f}%, Top5 Acc: {:.2f}%\n'.format(top1, top5)
    assert sorted(os.listdir(d)) == ["global_retrieval_acc.txt", "knn_acc.txt"]
    assert open(os.path.join(d, "global_retrieval_acc.txt")).read() == str(g["knn_%s/file" % dm])
    assert open(os.path.join(d, "knn_acc.txt")).read() == 'epoch:{} {:.2f} {:.2f}\n'.format(epoch, top1, top5)

    # KNN_K below 20 keeps the search at 20; KNN_WEIGHTS / KNN_T are read
    acc, out, K, d = run(ns(KNN_K=7, KNN_WEIGHTS='uniform', KNN_T=0.5), "on7")
    assert K.calls == [("search", 20, dm), ("label_hits", (40, 20), (1, 5, 10, 20)), ("vote", 7, UNIFORM, 5)]
    assert np.array_equal(acc, g["knn_%s/acc" % dm]) and 'kNN (k=7, uniform) Top1 Acc: ' in out
