"""GPU: slic_knn_vote and slic_retrieval_ranked (csrc/knn.hip) on hand-made tables against the float32 restatement and the float64
oracle of tests/knn_cpu_kernels.py, then neighbors.KNeighborsClassifier / evaluate.knn_classify / retrieval_metrics end to end through
the real searches on the sklearn goldens (tests/golden/knn.npz).  The host logic alone: tests/test_knn_cpu.py.

Bounds that no analysis fixes in advance are 4 x the largest difference measured on the MI355X over the cases of the test; the
measured value stands beside each bound (and in profiles/knn.txt)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_cases import RANKED_CASES, VOTE_CASES, ranked_case, vote_case      # noqa: E402

pytestmark = pytest.mark.gpu
TEMPERATURE = 0.07

# slic_knn_vote mode 2 on the hand-made tables, largest |proba - float64 oracle| over VOTE_CASES (expf on the device against np.exp)
SOFTMAX_TABLE_MEASURED = 1.3243e-07
SOFTMAX_TABLE_BOUND = 4 * SOFTMAX_TABLE_MEASURED
# predict_proba end to end on the goldens against the float64 oracle on float64 distances, largest difference over metric x k x precision
# (it reflects the float32 distances of the searches)
E2E_MEASURED = {"distance": 1.23382e-05, "softmax": 3.57548e-07}
E2E_BOUND = {w: 4 * v for w, v in E2E_MEASURED.items()}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "knn.npz")))


@pytest.fixture(scope="module")
def K(gpu):
    from video_similarity_search_amd.neighbors import HipKnnKernels
    return HipKnnKernels()


def device_vote(K, tab, C, mode, n_top):
    idx, dist, g_labels = tab
    proba, pred, score = K.vote(torch.from_numpy(idx).cuda(), torch.from_numpy(dist).cuda(), torch.from_numpy(g_labels).cuda(), C, mode,
                                TEMPERATURE, n_top, True)
    return proba.cpu().numpy(), pred.cpu().numpy(), score.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("k,Nq,C,n_top", VOTE_CASES)
@pytest.mark.parametrize("mode", [0, 1])
def test_vote_bit_identical(K, k, Nq, C, n_top, mode):
    """modes 0 and 1: proba (numerator and total in the kernel's order), pred and score equal the float32 restatement bit for bit"""
    from knn_cpu_kernels import vote32
    tab = vote_case(k, Nq, C)
    proba, pred, score = device_vote(K, tab, C, mode, n_top)
    p32, pred32, score32, s32 = vote32(*tab, C, mode, TEMPERATURE, n_top)
    assert np.array_equal(pred, pred32)
    assert np.array_equal(bits(score), bits(score32))
    assert np.array_equal(bits(proba), bits(p32))
    if C <= n_top:                                                      # every numerator is among the scores
        for q in range(Nq):
            live = pred[q] >= 0
            assert np.array_equal(bits(score[q][live]), bits(s32[q][pred[q][live]]))
    if Nq > 1:                                                          # the row of nothing but padding
        assert (proba[Nq - 1] == 0).all() and (pred[Nq - 1] == -1).all() and (score[Nq - 1] == 0).all()


def test_vote_optional_outputs(K):
    """each output alone gives what it gives together with the others; mode 0 needs no distance table"""
    idx, dist, g_labels = (torch.from_numpy(a).cuda() for a in vote_case(20, 5, 65))
    proba, pred, score = K.vote(idx, dist, g_labels, 65, 1, TEMPERATURE, 5, True)
    assert K.vote(idx, dist, g_labels, 65, 1, TEMPERATURE, 0, True)[1:] == (None, None)
    assert torch.equal(K.vote(idx, dist, g_labels, 65, 1, TEMPERATURE, 0, True)[0], proba)
    assert torch.equal(K.vote(idx, dist, g_labels, 65, 1, TEMPERATURE, 5, False)[1], pred)
    assert torch.equal(K.vote(idx, None, g_labels, 65, 0, TEMPERATURE, 5, False)[1], K.vote(idx, dist, g_labels, 65, 0, 1.0, 5, False)[1])
    from video_similarity_search_amd import _lib
    for bad in (dict(n_classes=4097), dict(n_classes=0), dict(mode=3), dict(n_top=9)):
        a = dict(n_classes=65, mode=1, n_top=5)
        a.update(bad)
        with pytest.raises(_lib.SlicError):
            K.vote(idx, dist, g_labels, a["n_classes"], a["mode"], TEMPERATURE, a["n_top"], True)
    with pytest.raises(_lib.SlicError):
        K.vote(idx, None, g_labels, 65, 1, TEMPERATURE, 5, True)        # a weighing mode without distances
    with pytest.raises(_lib.SlicError):
        K.vote(idx, dist, g_labels, 65, 2, 0.0, 5, True)                # temperature 0


def test_vote_softmax_vs_float64(K):
    """mode 2 against the float64 oracle over every hand-made table; the classes ranked are the oracle's wherever its scores are apart"""
    from knn_cpu_kernels import vote64
    worst = 0.0
    for (k, Nq, C, n_top) in VOTE_CASES:
        tab = vote_case(k, Nq, C)
        proba, pred, score = device_vote(K, tab, C, 2, n_top)
        p64, pred64, score64, s64 = vote64(*tab, C, 2, TEMPERATURE, n_top)
        worst = max(worst, float(np.abs(proba - p64).max()))
        assert ((pred >= 0) == (pred64 >= 0)).all()
        top2 = np.sort(s64, axis=1)[:, ::-1][:, :2] if C > 1 else np.concatenate([s64, s64 - 1], axis=1)
        sure = (top2[:, 0] - top2[:, 1]) > 1e-4 * np.maximum(top2[:, 0], 1e-30)
        assert np.array_equal(pred[sure, 0], pred64[sure, 0])
        assert np.allclose(score[:, 0], score64[:, 0], rtol=1e-4, atol=1e-30)
    print("slic_knn_vote mode 2: largest |proba - float64 oracle| over the hand-made tables = %.6g (bound %.6g)" % (worst, SOFTMAX_TABLE_BOUND))
    assert worst <= SOFTMAX_TABLE_BOUND


@pytest.mark.parametrize("k,Nq,ks", RANKED_CASES)
def test_ranked_vs_float64(K, k, Nq, ks):
    from knn_cpu_kernels import ranked64
    idx, ql, gl, n_rel = ranked_case(k, Nq, ks)
    per_query, rr, record = K.ranked(torch.from_numpy(idx).cuda(), torch.from_numpy(ql).cuda(), torch.from_numpy(gl).cuda(),
                                     torch.from_numpy(n_rel).cuda(), ks)
    pq64, rr64, rec64 = ranked64(idx, ql, gl, n_rel, ks)
    assert np.allclose(per_query.cpu().numpy(), pq64, rtol=1e-12, atol=0)
    assert np.allclose(rr.cpu().numpy(), rr64, rtol=1e-12, atol=0)
    assert np.allclose(record.cpu().numpy(), rec64, rtol=1e-12, atol=0)
    assert record[-1].item() == (n_rel > 0).sum()


def test_ranked_rejects_bad_cutoffs(K):
    from video_similarity_search_amd import _lib
    idx, ql, gl, n_rel = (torch.from_numpy(a).cuda() for a in ranked_case(20, 5, (1, 5)))
    for ks in ((5, 1), (0, 5), (1, 21), tuple(range(1, 10))):
        with pytest.raises(_lib.SlicError):
            K.ranked(idx, ql, gl, n_rel, ks)


E2E_CASES = [(m, p, k) for (m, p) in (("cosine", "fp32"), ("cosine", "bf16"), ("euclidean", "fp32")) for k in (1, 5, 20, 88)]


@pytest.mark.parametrize("metric,precision,k", E2E_CASES)
def test_classifier_end_to_end(gpu, golden, monkeypatch, metric, precision, k):
    """through the real searches: sklearn's labels on the queries that are not skipped, 'uniform' probabilities outright, 'distance' and
    'softmax' probabilities within the measured bound of the float64 oracle"""
    from video_similarity_search_amd.neighbors import KNeighborsClassifier
    from knn_cpu_kernels import DISTANCE, SOFTMAX, search64, vote64
    monkeypatch.setenv("SLIC_TOPK_BF16", "1")                           # precision='bf16' then runs the bf16 kernels wherever they can
    g = golden
    X, y, Q = g[metric + "/gallery"], g[metric + "/gallery_labels"], g[metric + "/queries"]
    classes, dense = np.unique(y, return_inverse=True)
    idx64, dist64 = search64(Q, X, k, metric)
    for weights in ("uniform", "distance", "softmax"):
        clf = KNeighborsClassifier(n_neighbors=k, weights=weights, metric=metric, temperature=TEMPERATURE, precision=precision).fit(X, y)
        proba = clf.predict_proba(Q)
        assert proba.is_cuda and tuple(proba.shape) == (96, 7)
        proba, pred = proba.cpu().numpy(), clf.predict(Q)
        if weights == "softmax":
            p64, top, _, _ = vote64(idx64, dist64, dense, 7, SOFTMAX, TEMPERATURE, 1)
            two = np.sort(p64, axis=1)[:, ::-1]
            skip = (two[:, 0] - two[:, 1]) < 1e-4
            want = classes[top[:, 0]]
        else:
            key = "%s/%s/%d/" % (metric, weights, k)
            skip, want = g[key + "skip"], g[key + "predict"]
        assert skip.mean() <= 0.02 and pred.dtype == y.dtype
        assert np.array_equal(pred[~skip], want[~skip])
        if weights == "uniform":
            assert np.array_equal(proba, g[key + "proba"].astype(np.float32))
        else:
            p64 = vote64(idx64, dist64, dense, 7, DISTANCE if weights == "distance" else SOFTMAX, TEMPERATURE, 0)[0]
            err = float(np.abs(proba - p64).max())
            print("predict_proba %s %s k=%d weights=%s: largest |proba - float64 oracle| = %.6g (bound %.6g)" % (
                metric, precision, k, weights, err, E2E_BOUND[weights]))
            assert err <= E2E_BOUND[weights]
    d, i = clf.kneighbors(Q)
    assert np.array_equal(np.sort(i.cpu().numpy(), axis=1), np.sort(idx64, axis=1))      # the gap at k: the same k rows as in float64


class SameTables(object):
    """the NumPy provider fed with the tables the device search returned: what is left to differ is the vote / the ranked metrics"""

    def __new__(cls, dev):
        from knn_cpu_kernels import NumpyKnnKernels

        class _P(NumpyKnnKernels):
            def search(self, x, y, k, dist_metric, precision="fp32"):
                self.calls.append(("search", int(k), dist_metric))
                idx, dist = dev.search(x, y, k, dist_metric, precision)
                return idx.cpu(), dist.cpu()
        return _P()


def same(a, b):
    """two result dicts: the same keys, the same numbers (torch's float64 sums on the two devices may differ in the last place)"""
    return set(a) == set(b) and all(np.isclose(a[key], b[key], rtol=1e-12, atol=0) for key in a)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_evaluate_functions_match_cpu_provider(K, golden, metric):
    from video_similarity_search_amd.evaluate import knn_classify, retrieval_metrics
    X, Q = golden[metric + "/gallery"], golden[metric + "/queries"]
    _, y = np.unique(golden[metric + "/gallery_labels"], return_inverse=True)
    _, yq = np.unique(golden[metric + "/query_labels"], return_inverse=True)
    yq = yq.copy()
    yq[5:9] = 50                                                        # queries without a relevant row
    for weights in ("uniform", "distance"):                             # bit-identical votes: the same accuracies
        dev = knn_classify(Q, yq, X, y, k=20, weights=weights, num_classes=7, dist_metric=metric)
        cpu = knn_classify(Q, yq, X, y, k=20, weights=weights, num_classes=7, dist_metric=metric, kernels=SameTables(K))
        assert same(dev, cpu) and dev["n_queries"] == 96 and dev["top1"] > 0.85
    dev = knn_classify(Q, yq, X, y, k=20, num_classes=7, dist_metric=metric)           # softmax: expf's last place can move a near-tie
    cpu = knn_classify(Q, yq, X, y, k=20, num_classes=7, dist_metric=metric, kernels=SameTables(K))
    assert all(abs(dev[key] - cpu[key]) <= 2.0 / 96 for key in cpu)
    loo_dev = knn_classify(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), k=5, weights="distance", dist_metric=metric)
    assert same(loo_dev, knn_classify(X, y, k=5, weights="distance", dist_metric=metric, kernels=SameTables(K)))
    ks = (1, 5, 10, 20, 50)
    dev = retrieval_metrics(Q, yq, X, y, ks=ks, dist_metric=metric)
    cpu = retrieval_metrics(Q, yq, X, y, ks=ks, dist_metric=metric, kernels=SameTables(K))
    assert dev["n_with_relevant"] == cpu["n_with_relevant"] == 92 and np.isclose(dev["mrr"], cpu["mrr"], rtol=1e-12)
    for name in ("precision", "recall", "map"):
        assert all(np.isclose(dev[name][k], cpu[name][k], rtol=1e-12) for k in ks)
    loo = retrieval_metrics(X, y, ks=(1, 5), dist_metric=metric)
    cpu = retrieval_metrics(X, y, ks=(1, 5), dist_metric=metric, kernels=SameTables(K))
    assert loo["n_with_relevant"] == 600 and np.isclose(loo["map"][5], cpu["map"][5], rtol=1e-12)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_leave_one_out_excludes_self(gpu, golden, metric):
    from video_similarity_search_amd.neighbors import KNeighborsClassifier, NearestNeighbors
    X, y = golden[metric + "/gallery"], golden[metric + "/gallery_labels"]
    dist, idx = NearestNeighbors(n_neighbors=5, metric=metric).fit(X).kneighbors()
    assert idx.is_cuda and not (idx.cpu().numpy() == np.arange(600)[:, None]).any()
    assert np.array_equal(idx.cpu().numpy(), golden[metric + "/loo_idx"])
    # duplicated rows: the copy is a neighbour at distance 0, the row itself still is not
    X2 = np.concatenate([X[:50], X[:50]])
    dist, idx = NearestNeighbors(n_neighbors=3, metric=metric).fit(X2).kneighbors()
    idx = idx.cpu().numpy()
    assert not (idx == np.arange(100)[:, None]).any() and np.array_equal(idx[:, 0], (np.arange(100) + 50) % 100)
    clf = KNeighborsClassifier(n_neighbors=3, weights="distance", metric=metric).fit(X2, np.concatenate([y[:50], y[:50]]))
    assert np.array_equal(clf.predict(), np.concatenate([y[:50], y[:50]]))     # the zero-distance rule: the copy decides
