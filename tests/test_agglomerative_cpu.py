"""CPU: the agglomerative host driver (round loop, fallback, termination), fit_cluster's 'Agglomerative' method and the argument errors,
run against the NumPy provider (tests/agglo_cpu_kernels.py) and the sklearn goldens (tests/golden/agglomerative.npz); the device path is
test_agglomerative_gpu.py."""
import numpy as np
import pytest
import torch

from agglo_cpu_kernels import NumpyAggloKernels, agglo_fp64, canonical, golden_cases, oracle_gap


def _model(**kw):
    from video_similarity_search_amd.clustering import AgglomerativeClustering
    return AgglomerativeClustering(**kw)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_fp64_oracle_reproduces_goldens(case):
    name, X, t, labels = case
    got, heights, last = agglo_fp64(X, t)
    assert got.dtype == np.int32 and np.array_equal(got, labels), name
    assert len(heights) == len(X) - (labels.max() + 1)                 # every merge removes one cluster
    assert np.all(heights < t) and not last < t
    assert oracle_gap(heights, last, t) >= 1e-4                        # what the goldens were picked for


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_driver_reproduces_goldens(case):
    name, X, t, labels = case
    m = _model(distance_threshold=t, kernels=NumpyAggloKernels(np.float32)).fit(X)
    assert m.labels_.dtype == np.int32 and m.labels_.shape == (len(X),)
    assert np.array_equal(m.labels_, labels), name
    assert m.n_clusters_ == labels.max() + 1 and m.n_leaves_ == len(X)
    if len(X) > 1:
        assert m.rounds_ >= 1 and len(X) <= m.n_query_rows_ <= m.rounds_ * len(X)
    else:
        assert m.rounds_ == 0 and m.n_query_rows_ == 0
    assert np.array_equal(_model(distance_threshold=t, affinity='cosine', kernels=NumpyAggloKernels()).fit(torch.from_numpy(X)).labels_, labels)


def test_goldens_cover_the_cases():
    cases = {c[0]: c for c in golden_cases()}
    _, X, t, labels = cases["blobs16_t024"]
    dup = np.flatnonzero((X == X[7]).all(axis=1))
    assert len(dup) == 3 and len(set(labels[dup])) == 1                # the two exact duplicates of row 7 sit with it
    assert cases["blobs16_t010"][3].max() > labels.max() > 3           # several merge levels: the lower cut is finer
    assert np.bincount(cases["blobs128_t06"][3]).max() >= 0.95 * len(cases["blobs128_t06"][1])
    assert np.array_equal(cases["noise_120x32"][3], np.arange(120))
    assert cases["two_rows_merge"][3].tolist() == [0, 0] and cases["two_rows_apart"][3].tolist() == [0, 1]
    assert cases["one_row"][3].tolist() == [0]
    assert canonical([5, 5, 2, 9, 2]).tolist() == [0, 0, 1, 2, 1]


def test_stale_only_search_saves_queries():
    _, X, t, labels = [c for c in golden_cases() if c[0] == "blobs16_t024"][0]
    m = _model(distance_threshold=t, kernels=NumpyAggloKernels()).fit(X)
    assert m.rounds_ > 3 and m.n_query_rows_ < m.rounds_ * len(X) / 2


class _CycleKernels(NumpyAggloKernels):
    """a provider whose first search answers with a 3-cycle 0 -> 1 -> 2 -> 0 at last-bit-different distances: no reciprocal pair"""

    def __init__(self):
        super().__init__(np.float64)
        self.calls = 0

    def search(self, Mq, M, own):
        pos, dist = super().search(Mq, M, own)
        self.calls += 1
        if self.calls == 1:
            pos[:3] = [1, 2, 0]
            dist[:3] = [0.0100002, 0.0100001, 0.0100003]
        return pos, dist


def test_fallback_merges_the_closest_pair_of_a_cycle():
    # three rows at 120 degrees in a plane (every pair equally far in exact arithmetic) next to a far fourth row
    ang = np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3])
    X = np.zeros((4, 3), np.float32)
    X[:3, 0], X[:3, 1], X[:3, 2] = np.cos(ang) * 0.1, np.sin(ang) * 0.1, 1.0
    X[3] = [1.0, 0.0, -1.0]
    k = _CycleKernels()
    m = _model(distance_threshold=0.1, kernels=k).fit(X)
    assert m.n_fallback_merges_ == 1
    assert k.heights[0] == 0.0100001 and k.parent[2] == 1            # the closest link of the cycle, 1 -> 2, merged first; the lower id survives
    assert m.labels_.tolist() == [0, 0, 0, 1] and m.n_clusters_ == 2   # and the run went on to the greedy result
    assert m.rounds_ <= 4


def test_every_round_merges_or_ends():
    """duplicates: a star under lowest-index tie-breaking, m - 1 rounds for m identical rows, never more"""
    X = np.tile(np.random.default_rng(0).standard_normal((1, 8)).astype(np.float32), (9, 1))
    m = _model(distance_threshold=0.24, kernels=NumpyAggloKernels()).fit(X)
    assert m.n_clusters_ == 1 and m.labels_.tolist() == [0] * 9 and m.rounds_ <= 9
    m = _model(distance_threshold=0.0, kernels=NumpyAggloKernels()).fit(X)
    assert m.n_clusters_ == 9 and m.rounds_ == 1                       # d < 0 never holds: one round, nothing merges


def test_fit_cluster_agglomerative_prints_and_returns(capsys):
    from video_similarity_search_amd.clustering import fit_cluster
    name, X, t, labels = [c for c in golden_cases() if c[0] == "blobs16_t024"][0]
    out = fit_cluster(torch.from_numpy(X), 'Agglomerative', distance_threshold=0.24, kernels=NumpyAggloKernels())
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, labels)
    assert capsys.readouterr().out.splitlines() == ["Clustering with Agglomerative...", str((len(X),)),
                                                    "Fitted {} clusters with Agglomerative".format(labels.max() + 1)]
    out = fit_cluster(X, 'Agglomerative', distance_threshold=0.1, l2normalize=False, kernels=NumpyAggloKernels())
    assert np.array_equal(out, [c for c in golden_cases() if c[0] == "blobs16_t010"][0][3])


def test_argument_errors():
    from video_similarity_search_amd.clustering import fit_cluster
    X = np.random.default_rng(1).standard_normal((6, 4)).astype(np.float32)
    k = NumpyAggloKernels
    with pytest.raises(NotImplementedError, match="metric"):
        _model(metric='euclidean', distance_threshold=0.2, kernels=k()).fit(X)
    with pytest.raises(NotImplementedError, match="metric"):
        _model(affinity='l2', distance_threshold=0.2, kernels=k()).fit(X)
    with pytest.raises(NotImplementedError, match="linkage"):
        _model(linkage='ward', distance_threshold=0.2, kernels=k()).fit(X)
    with pytest.raises(NotImplementedError, match="n_clusters"):
        _model(n_clusters=3, kernels=k()).fit(X)
    with pytest.raises(ValueError, match="distance_threshold"):
        _model(kernels=k()).fit(X)
    Z = X.copy()
    Z[2] = 0
    with pytest.raises(ValueError, match="zero norm"):
        _model(distance_threshold=0.2, kernels=k()).fit(Z)
    Z[2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        _model(distance_threshold=0.2, kernels=k()).fit(Z)
    with pytest.raises(ValueError):
        _model(distance_threshold=0.2, kernels=k()).fit(np.zeros((1, 4), np.float32))
    # the bare call names the keyword; OPTICS still raises
    with pytest.raises(NotImplementedError, match="distance_threshold"):
        fit_cluster(X, 'Agglomerative')
    with pytest.raises(NotImplementedError):
        fit_cluster(X, 'OPTICS', distance_threshold=0.24)


def test_no_device_raises():
    from video_similarity_search_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.SlicError):
        _model(distance_threshold=0.24).fit(torch.randn(64, 8))
    from video_similarity_search_amd.clustering import fit_cluster
    with pytest.raises(_lib.SlicError):
        fit_cluster(torch.randn(64, 8), 'Agglomerative', distance_threshold=0.24)
