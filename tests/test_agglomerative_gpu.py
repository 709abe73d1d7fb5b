"""GPU: csrc/agglo.hip behind AgglomerativeClustering — the sklearn goldens, the float64 round oracle (tests/agglo_cpu_kernels.py) at the
smallest shapes where the scan blocks (1024 ids), the search tiles (128 rows), the column padding (D % 8) and the 256-column lane stride
have edges, the degenerate thresholds, duplicates, input kinds, determinism, the stale-only search and the memory bound."""
import functools

import numpy as np
import pytest
import torch

from agglo_cpu_kernels import agglo_fp64, blobs, golden_cases, oracle_gap

pytestmark = pytest.mark.gpu

GAP = 1e-4      # an fp32 dot product of two means at D <= 512 is off by at most ~D * 6e-8 = 3e-5; the oracle clears that threefold

# (N, D, threshold, blobs(seed, N, D, centres, spread, sub, subspread)): seeds picked on the CPU so that the oracle's gap is >= GAP
ORACLE_CASES = [
    (2, 8, 0.24, (0, 1, 0.3, 0, 0.0)),               # the two rows merge
    (2, 8, 0.05, (0, 1, 0.6, 0, 0.0)),               # and stay apart
    (3, 8, 0.24, (1, 1, 0.4, 0, 0.0)),
    (129, 5, 0.05, (1, 6, 0.35, 0, 0.0)),
    (257, 20, 0.15, (0, 5, 0.3, 4, 0.5)),
    (1000, 128, 0.2, (2, 8, 0.45, 5, 0.45)),
    (3000, 512, 0.24, (0, 10, 0.5, 6, 0.25)),        # 21 merge heights within 0.01 of the threshold
    (6000, 128, 0.2, (2, 12, 0.45, 8, 0.45)),
]


@functools.lru_cache(maxsize=None)
def oracle(case):
    N, D, t, (seed, centres, spread, sub, subspread) = case
    X = blobs(seed, N, D, centres, spread, sub, subspread)
    labels, heights, last = agglo_fp64(X, t)
    X.setflags(write=False)
    labels.setflags(write=False)
    return X, labels, oracle_gap(heights, last, t)


@functools.lru_cache(maxsize=None)
def fitted(case):
    from video_similarity_search_amd.clustering import AgglomerativeClustering
    X, _, _ = oracle(case)
    return AgglomerativeClustering(distance_threshold=case[2]).fit(torch.tensor(X).cuda())


def _fit(X, t):
    from video_similarity_search_amd.clustering import AgglomerativeClustering
    return AgglomerativeClustering(distance_threshold=t).fit(X)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_goldens(gpu, case):
    name, X, t, labels = case
    m = _fit(X, t)
    assert m.labels_.dtype == np.int32 and np.array_equal(m.labels_, labels), name
    assert m.n_clusters_ == labels.max() + 1 and m.n_leaves_ == len(X)


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: "{}x{}_t{}".format(*c[:3]))
def test_matches_fp64_oracle(gpu, case):
    X, labels, gap = oracle(case)
    print("oracle gap", gap, "clusters", labels.max() + 1)
    assert gap >= GAP                                   # asserted on the CPU first: the case is decidable in fp32
    m = fitted(case)
    print("rounds", m.rounds_, "query rows", m.n_query_rows_, "fallback merges", m.n_fallback_merges_)
    assert np.array_equal(m.labels_, labels)
    assert m.n_clusters_ == labels.max() + 1


def test_cases_are_not_trivial():
    for case in ORACLE_CASES[3:]:
        _, labels, _ = oracle(case)
        assert 1 < labels.max() + 1 < case[0] / 1.5 and np.bincount(labels).max() > 2
    assert oracle(ORACLE_CASES[0])[1].tolist() == [0, 0] and oracle(ORACLE_CASES[1])[1].tolist() == [0, 1]


def test_threshold_extremes(gpu):
    X = blobs(5, 300, 16, 4, 0.3)
    m = _fit(X, 2.0)
    assert m.n_clusters_ == 1 and not m.labels_.any()
    m = _fit(X, 0.0)
    assert m.n_clusters_ == 300 and m.rounds_ == 1 and np.array_equal(m.labels_, np.arange(300))


def test_identical_rows(gpu):
    X = np.tile(np.random.default_rng(3).standard_normal((1, 24)).astype(np.float32), (64, 1))
    m = _fit(X, 0.24)
    assert m.n_clusters_ == 1 and not m.labels_.any() and m.rounds_ <= 64


def test_input_kinds_and_determinism(gpu):
    case = ORACLE_CASES[5]
    X, labels, _ = oracle(case)
    ref = fitted(case)
    dev = torch.tensor(X).cuda()
    keep = dev.clone()
    again = _fit(dev, case[2])
    assert torch.equal(dev, keep)                                          # a device tensor is used in place and left as it was
    assert again.labels_.tobytes() == ref.labels_.tobytes()                # two runs: the same bits
    assert (again.rounds_, again.n_query_rows_) == (ref.rounds_, ref.n_query_rows_)
    assert np.array_equal(_fit(torch.tensor(X), case[2]).labels_, ref.labels_)
    assert np.array_equal(_fit(X, case[2]).labels_, ref.labels_)
    wide = torch.zeros(len(X), X.shape[1] + 3, device="cuda")
    wide[:, :X.shape[1]] = dev
    assert np.array_equal(_fit(wide[:, :X.shape[1]], case[2]).labels_, ref.labels_)     # a row stride beyond D


def test_bad_rows_raise(gpu):
    X = blobs(7, 40, 12, 3, 0.3)
    X[17] = 0
    with pytest.raises(ValueError, match="1 row"):
        _fit(X, 0.24)
    X[17, 3] = np.inf
    X[2, 0] = np.nan
    with pytest.raises(ValueError, match="2 row"):
        _fit(torch.tensor(X).cuda(), 0.24)


def test_fit_cluster_on_device(gpu, capsys):
    from video_similarity_search_amd.clustering import fit_cluster
    case = ORACLE_CASES[4]
    X, labels, _ = oracle(case)
    out = fit_cluster(torch.tensor(X).cuda(), 'Agglomerative', distance_threshold=case[2])
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, labels)
    assert capsys.readouterr().out.splitlines() == ["Clustering with Agglomerative...", str((len(X),)),
                                                    "Fitted {} clusters with Agglomerative".format(labels.max() + 1)]


def test_stale_only_search_is_active(gpu):
    m = fitted(ORACLE_CASES[7])
    print("rounds", m.rounds_, "query rows", m.n_query_rows_)
    assert m.n_query_rows_ < m.rounds_ * 6000 / 2


def test_memory_stays_linear(gpu):
    """N = 8192, D = 64: an N x N fp32 matrix would be 268 MB; rows, sums, means and the top-2 workspace come to a few MB"""
    X = blobs(11, 8192, 64, 16, 0.45, 6, 0.4)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = _fit(X, 0.2)
    peak = torch.cuda.max_memory_allocated() - base
    print("peak bytes over the fit", peak, "clusters", m.n_clusters_, "rounds", m.rounds_)
    assert 1 < m.n_clusters_ < 8192
    assert peak < 64 * 2 ** 20
