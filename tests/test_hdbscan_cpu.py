"""CPU: HDBSCAN's host side.  The float64 restatement (tests/hdbscan_cpu_kernels.py) against the sklearn goldens
(tests/golden/hdbscan.npz: labels and probabilities on the rows that are stable under row permutations, see the generator), the driver
with the NumPy provider against that restatement, Boruvka through the provider against Kruskal on the same fp32 weights, four defects
injected one at a time, fit_cluster's 'HDBSCAN' method, and the workspace query's rejections; the device path is test_hdbscan_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hdbscan_cpu_kernels import (NumpyHdbscanKernels, core_fp64, cut_fp64, distances_fp64, hdbscan_fp64, hdbscan_tree_fp64, is_spanning_tree,
                                 kruskal, mutual_reachability, prim_weights, same_partition)


def golden_cases():
    z = np.load(os.path.join(GOLDEN, "hdbscan.npz"))
    out = []
    for n in sorted({k.split("__")[0] for k in z.files}):
        mcs, ms, leaf, single = (int(v) for v in z[n + "__params"])
        out.append(dict(name=n, X=z[n + "__X"], mcs=mcs, ms=None if ms < 0 else ms, method='leaf' if leaf else 'eom', single=bool(single),
                        eps=float(z[n + "__eps"]), labels=z[n + "__labels"], prob=z[n + "__prob"], stable=z[n + "__stable"],
                        cuts=[(float(c), z[n + "__cut{}".format(i)]) for i, c in enumerate(z[n + "__cuts"])]))
    return out


def _fit(c, kernels, X=None):
    from video_similarity_search_amd.clustering.hdbscan import HDBSCAN
    return HDBSCAN(min_cluster_size=c["mcs"], min_samples=c["ms"], cluster_selection_method=c["method"], allow_single_cluster=c["single"],
                   cluster_selection_epsilon=c["eps"], kernels=kernels).fit(c["X"] if X is None else X)


def test_goldens_cover_the_cases():
    cases = {c["name"]: c for c in golden_cases()}
    assert len(cases) == 9 and all(len(c["X"]) <= 500 and c["X"].shape[1] == 32 for c in cases.values())
    assert {(c["mcs"], c["ms"], c["method"]) for c in cases.values()} >= {(5, None, 'eom'), (5, 2, 'eom'), (10, 3, 'eom'), (3, 3, 'eom'),
                                                                         (5, 2, 'leaf'), (8, 4, 'leaf')}
    assert any(c["eps"] > 0 for c in cases.values()) and any(c["single"] for c in cases.values())
    assert sum(len(c["cuts"]) for c in cases.values()) == 2
    X = cases["dup_mcs5_ms2"]["X"]
    assert np.array_equal(X[17], X[3])
    one = cases["one_single_mcs5_ms2"]["labels"]
    assert set(one.tolist()) == {-1, 0}
    for c in cases.values():
        assert (~c["stable"]).sum() <= 0.02 * len(c["X"])
        if (c["mcs"] if c["ms"] is None else c["ms"]) == 2:
            assert c["stable"].all()
    assert any(not c["stable"].all() for c in cases.values())


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_oracle_reproduces_sklearn(case):
    o = hdbscan_fp64(case["X"], case["mcs"], case["ms"], case["method"], case["single"], case["eps"])
    st = case["stable"]
    assert same_partition(o["labels"][st], case["labels"][st])
    assert np.all(np.abs(o["probabilities"] - case["prob"])[st] <= 1e-9)
    if st.all():
        assert same_partition(o["labels"], case["labels"])
    for cut, want in case["cuts"]:
        assert same_partition(cut_fp64(o["edges"], o["weights"], len(case["X"]), cut, case["mcs"]), want)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_driver_with_numpy_provider_equals_oracle(case):
    N = len(case["X"])
    m = _fit(case, NumpyHdbscanKernels())
    o = hdbscan_fp64(case["X"], case["mcs"], case["ms"], case["method"], case["single"], case["eps"])
    assert m.labels_.dtype == np.int32 and m.labels_.shape == (N,) and m.probabilities_.dtype == np.float64
    assert m.mst_edges_.dtype == np.int32 and m.mst_edges_.shape == (N - 1, 2) and m.mst_weights_.dtype == np.float64
    assert is_spanning_tree(m.mst_edges_, N)
    # the provider searches in fp32: its tree is the oracle's up to the fp32 error of a score, (Dp + 2) 2^-24
    assert np.all(np.abs(m.mst_weights_ - o["weights"]) <= 2 * 34 * 2.0 ** -24)
    st = case["stable"]
    assert same_partition(m.labels_[st], o["labels"][st])
    # the host part alone, on the same tree: equal to the oracle's row-list form
    labels, prob = hdbscan_tree_fp64(m.mst_edges_, m.mst_weights_, N, case["mcs"], case["method"], case["single"], case["eps"])
    assert np.array_equal(labels, m.labels_) and np.all(np.abs(prob - m.probabilities_) <= 1e-12)
    assert m.n_clusters_ == int(m.labels_.max()) + 1
    assert np.all(np.abs(m.core_distances_ - o["core"]) <= 2 * 34 * 2.0 ** -24)
    for cut, want in case["cuts"]:
        assert same_partition(m.dbscan_clustering(cut, case["mcs"]), want)
    assert m.stats_["rounds"] <= int(np.ceil(np.log2(N))) and "seconds_host_tree" in m.stats_


def _small(seed=5, N=160, D=12):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((4, D))
    X = cen[rng.integers(0, 4, N)] + 0.3 * rng.standard_normal((N, D))
    X[:20] = rng.standard_normal((20, D))
    X[33] = X[7]                                                       # exact duplicates: w = 0 ties
    X[90] = 0.0                                                        # a zero row
    return (X * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)


@pytest.mark.parametrize("ms", [1, 2, 3, 5])
def test_provider_mirrors_the_entry_points_and_boruvka_is_canonical(ms):
    X = _small()
    N = len(X)
    k = NumpyHdbscanKernels()
    rows = k.resident(X)
    core = k.core_distances(rows, ms)
    d = distances_fp64(X)
    b = 2 * (16 + 2) * 2.0 ** -24
    assert np.all(np.abs(core - core_fp64(d, ms)) <= b)                # rule 2, the diagonal zero counted
    if ms == 1:
        assert np.all(core == 0.0)
    W32 = k.weights32()
    assert np.array_equal(W32, W32.T)
    edges, w = k.mst(rows, core)
    # Boruvka's candidates, merged by the host, are exactly rule 4's tree of the weights the rounds saw
    want, _ = kruskal(W32)
    assert np.array_equal(edges[np.lexsort((edges[:, 1], edges[:, 0]))], want[np.lexsort((want[:, 1], want[:, 0]))])
    # ... reported with rule 3's float64 weights, in tree order
    assert np.array_equal(w, np.maximum(d[edges[:, 0], edges[:, 1]], np.maximum(core[edges[:, 0]], core[edges[:, 1]])))
    assert np.all(np.diff(w) >= 0)
    assert np.all(np.abs(np.sort(w) - prim_weights(mutual_reachability(d, core_fp64(d, ms)))) <= b)
    assert k.last_stats["rounds"] <= int(np.ceil(np.log2(N)))
    # one round, every row its own component: the lightest foreign row, a tie to the smaller row
    lo, hi, ww = k.round(rows, np.arange(N, dtype=np.int32), N)
    Wm = W32.astype(np.float64)
    np.fill_diagonal(Wm, np.inf)
    j = np.argmin(Wm, axis=1)
    assert np.array_equal(lo, np.minimum(np.arange(N), j)) and np.array_equal(hi, np.maximum(np.arange(N), j))
    assert np.array_equal(ww, W32[np.arange(N), j])


@pytest.mark.parametrize("defect", ["no_diagonal", "larger_j", "no_mask", "keep_cycles"])
def test_injected_defects_are_caught(defect):
    """the checks above, applied to a provider with one deliberate error, must fail"""
    X = _small()
    N = len(X)
    ms = 3
    d = distances_fp64(X)
    good = NumpyHdbscanKernels()
    bad = NumpyHdbscanKernels(defect=defect)
    core = good.core_distances(good.resident(X), ms)
    bcore = bad.core_distances(bad.resident(X), ms)
    if defect == "no_diagonal":
        assert np.abs(bcore - core_fp64(d, ms)).max() > 1e-3            # the core check
        return
    assert np.array_equal(core, bcore)
    want, _ = kruskal(good.weights32())
    if defect == "no_mask":
        with pytest.raises(RuntimeError):                                # no candidate leaves its component: the rounds cannot end
            bad.mst(bad.resident(X), bcore)
        return
    edges, w = bad.mst(bad.resident(X), bcore)
    if defect == "keep_cycles":
        assert not is_spanning_tree(edges, N)                           # the tree check
        return
    assert is_spanning_tree(edges, N)                                   # larger_j: still a tree, not rule 4's
    assert not np.array_equal(edges[np.lexsort((edges[:, 1], edges[:, 0]))], want[np.lexsort((want[:, 1], want[:, 0]))])


def test_fit_cluster_hdbscan_prints_and_returns(capsys):
    from video_similarity_search_amd.clustering import fit_cluster
    case = [c for c in golden_cases() if c["name"] == "a_mcs5_ms2"][0]
    X = case["X"]
    out = fit_cluster(torch.from_numpy(X), 'HDBSCAN', min_cluster_size=5, min_samples=2, kernels=NumpyHdbscanKernels())
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and same_partition(out, case["labels"])
    n = int(case["labels"].max()) + 1
    assert capsys.readouterr().out.splitlines() == ["Clustering with HDBSCAN...", str((len(X),)), "Fitted {} clusters with HDBSCAN".format(n)]
    assert fit_cluster.last_model.n_clusters_ == n
    # min_samples=None is min_cluster_size; l2normalize does not apply
    case = [c for c in golden_cases() if c["name"] == "a_mcs5"][0]
    out = fit_cluster(3.0 * X, 'HDBSCAN', l2normalize=False, kernels=NumpyHdbscanKernels())
    assert same_partition(out[case["stable"]], case["labels"][case["stable"]])


def test_raises():
    from video_similarity_search_amd.clustering.hdbscan import HDBSCAN
    X = _small()
    k = NumpyHdbscanKernels
    for kw, word in ((dict(metric='euclidean'), "metric"), (dict(alpha=0.5), "alpha"), (dict(max_cluster_size=50), "max_cluster_size"),
                     (dict(store_centers='centroid'), "store_centers"), (dict(algorithm='kd_tree'), "algorithm"),
                     (dict(min_samples=89), "min_samples")):
        with pytest.raises(NotImplementedError, match=word):
            HDBSCAN(kernels=k(), **kw).fit(X)
    with pytest.raises(ValueError, match="n_samples=1 while HDBSCAN requires more than one sample"):
        HDBSCAN(kernels=k()).fit(X[:1])
    with pytest.raises(ValueError, match=r"min_samples \(7\) must be at most the number of samples in X \(6\)"):
        HDBSCAN(min_samples=7, kernels=k()).fit(X[:6])
    bad = X.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        HDBSCAN(kernels=k()).fit(bad)
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        HDBSCAN(kernels=k()).fit(torch.from_numpy(bad))
    for kw in (dict(min_cluster_size=1), dict(min_samples=0), dict(cluster_selection_epsilon=-1.0), dict(cluster_selection_method='xi')):
        with pytest.raises(ValueError):
            HDBSCAN(kernels=k(), **kw).fit(X)
    m = HDBSCAN(algorithm='brute', kernels=k())
    assert np.array_equal(m.fit_predict(X), m.labels_)
    two = HDBSCAN(min_cluster_size=2, min_samples=1, kernels=k()).fit(X[:2])           # the smallest fit there is
    assert two.mst_edges_.tolist() == [[0, 1]] and two.labels_.tolist() == [-1, -1]


def test_no_device_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from video_similarity_search_amd import _lib
    from video_similarity_search_amd.clustering import HDBSCAN, fit_cluster
    with pytest.raises(_lib.SlicError):
        fit_cluster(torch.randn(64, 8), 'HDBSCAN')
    with pytest.raises(_lib.SlicError):
        HDBSCAN().fit(np.ones((8, 4), np.float32))


def test_workspace_query_rejections():
    """no device work: the size query answers anywhere, 0 for what the entry points reject"""
    from video_similarity_search_amd import _lib
    f = _lib.load().slic_hdbscan_workspace_bytes
    assert f(1000, 128, 5) > 0 and f(2, 1, 1) > 0 and f(1000, 512, 88) > 0
    assert f(1000, 128, 5) < 1000 * 128 * 4 * 3                         # O(N Dp + N min_samples): no N x N
    for N, D, ms in ((1, 8, 1), (0, 8, 1), (1000, 0, 5), (1000, 513, 5), (1000, 8, 0), (1000, 8, 89), (4, 8, 5), (1 << 31, 8, 5),
                     (3_000_000, 512, 5)):                              # the last: >= 4 GiB padded
        assert f(N, D, ms) == 0, (N, D, ms)
    out = (ctypes.c_double * 6)()
    assert _lib.load().slic_hdbscan_stats(out) == 0


def test_cluster_step_silhouette_line_leaves_hdbscan_noise_out(capsys):
    """the opt-in silhouette line of the cluster step: -1 is noise for 'HDBSCAN' as it is for 'DBSCAN'"""
    import types
    from silhouette_cpu_kernels import NumpySilhouetteKernels, silhouette_fp64
    from video_similarity_search_amd.online_train import _silhouette_lines
    case = [c for c in golden_cases() if c["name"] == "a_mcs5_ms2"][0]
    X, labels = case["X"], case["labels"]
    assert (labels == -1).any()
    ns = types.SimpleNamespace
    _silhouette_lines(ns(OUTPUT_PATH=None, ITERCLUSTER=ns(METHOD='HDBSCAN')), 0, X, labels, NumpySilhouetteKernels())
    want = silhouette_fp64(X, labels, "cosine", ignore_label=-1)["score"]
    assert abs(want - silhouette_fp64(X, labels, "cosine")["score"]) > 5e-3          # the noise rows as a cluster: another score
    assert capsys.readouterr().out == "Silhouette (cosine) of the cluster assignments: {:.3f}\n".format(want)
