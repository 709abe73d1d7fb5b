"""GPU: DBSCAN (cosine) on the device (csrc/dbscan.hip) against the sklearn goldens and the float64 oracle
(tests/dbscan_cpu_kernels.py): counts, core flags and labels equal, the float64 recheck deciding every pair in the screening
band, degenerate inputs (identical rows, orthogonal rows, eps >= 2, one row, zero rows), determinism and input forms."""
import time

import numpy as np
import pytest
import torch

from dbscan_cpu_kernels import dbscan_fp64, inv_norms
from test_dbscan_cpu import golden_cases

pytestmark = pytest.mark.gpu


def _fit(X, eps, ms):
    from video_similarity_search_amd.clustering.dbscan import DBSCAN
    return DBSCAN(eps=eps, min_samples=ms).fit(X)


def _blobs(seed, N, D, K, spread, noise_frac=0.1):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((K, D))
    sp = spread * rng.uniform(0.5, 1.5, K)
    y = rng.integers(0, K, N)
    X = cen[y] + sp[y, None] * rng.standard_normal((N, D)) * np.sqrt(16.0 / D)
    nn = int(noise_frac * N)
    X[:nn] = rng.standard_normal((nn, D))
    return X[rng.permutation(N)].astype(np.float32)


def _check_against_oracle(X, eps, ms):
    m = _fit(torch.from_numpy(X).cuda(), eps, ms)
    labels, core, counts, ncl = dbscan_fp64(X, eps, ms)
    assert np.array_equal(m.n_neighbors_, counts)
    assert np.array_equal(m.core_sample_indices_, np.flatnonzero(core))
    assert np.array_equal(m.labels_, labels)
    assert m.n_clusters_ == ncl
    return m


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_goldens_exact(gpu, case):
    name, X, eps, ms, labels, core = case
    m = _fit(X, eps, ms)
    assert np.array_equal(m.labels_, labels), name
    assert np.array_equal(m.core_sample_indices_, core), name
    assert m.n_clusters_ == len(set(labels.tolist()) - {-1})


@pytest.mark.parametrize("N,D,eps,ms", [
    (3000, 8, 0.05, 2), (20000, 8, 0.05, 3), (5000, 100, 0.14, 5), (8000, 128, 0.14, 2), (6000, 128, 0.3, 3),
    (4000, 512, 0.14, 3), (3000, 512, 0.3, 5), (12000, 100, 0.3, 2),
    (3000, 200, 0.3, 3), (3000, 320, 0.3, 3),                        # db_tiles<NK = 8> and <NK = 12>
])
def test_matches_fp64_oracle(gpu, N, D, eps, ms):
    X = _blobs(N + D, N, D, K=max(4, N // 400), spread=0.15 if eps < 0.1 else 0.3)
    m = _check_against_oracle(X, eps, ms)
    assert m.n_clusters_ > 1 and (m.labels_ == -1).any()


# N -> seed of _blobs: N + 8 where the float64 oracle alone then has core rows, border candidates and noise rows, else the next that has
SCAN_SEEDS = {1: 9, 2: 10, 63: 71, 64: 73, 65: 74, 1023: 1032, 1024: 1032, 1025: 1033, 2049: 2057}


@pytest.mark.parametrize("N", sorted(SCAN_SEEDS))
def test_matches_fp64_oracle_at_the_scan_sizes(gpu, N):
    """the one-workgroup scans of db_compact and db_number (1024 threads, runs of ceil(N / 1024) rows): a partly filled last wave, empty
    trailing runs, runs of 1 next to runs of 2; all three outputs of the compaction non-empty from N = 63 on"""
    D, eps, ms = 8, 0.05, 3
    X = _blobs(SCAN_SEEDS[N], N, D, K=max(4, N // 400), spread=0.15)
    labels, core, counts, ncl = dbscan_fp64(X, eps, ms)
    if N >= 63:
        assert core.any() and ((counts >= 2) & ~core).any() and (labels == -1).any()
    _check_against_oracle(X, eps, ms)


def test_screening_band_decided_in_fp64(gpu):
    """chains of rows in disjoint 2-D planes: consecutive rows sit within 1e-7 of the eps boundary on either side (fp32 cannot
    tell), non-consecutive ones far away; counts, cores and labels must be the float64 decision's"""
    eps, D = 0.005, 128
    th0 = np.arccos(1.0 - eps)
    rng = np.random.default_rng(7)
    rows = []
    for pl in range(D // 2):
        shift = rng.uniform(-1e-7, 1e-7, 39) / np.sin(th0)         # d(step) = eps + ~U(-1e-7, 1e-7)
        ang = np.concatenate([[0.0], np.cumsum(th0 + shift)])
        r = np.zeros((40, D))
        r[:, 2 * pl], r[:, 2 * pl + 1] = np.cos(ang), np.sin(ang)
        rows.append(r * rng.uniform(0.5, 2.0, (40, 1)))
    X = np.concatenate(rows).astype(np.float32)
    from video_similarity_search_amd.clustering.dbscan import DBSCAN
    for ms in (2, 3):
        labels, core, counts, ncl = dbscan_fp64(X, eps, ms)
        assert (counts == 1).any() and (counts == 3).any()           # both sides of the boundary occur
        m = DBSCAN(eps=eps, min_samples=ms).fit(torch.from_numpy(X).cuda())
        assert np.array_equal(m.n_neighbors_, counts)
        assert np.array_equal(m.core_sample_indices_, np.flatnonzero(core))
        assert np.array_equal(m.labels_, labels)
        assert m.stats_["band_rechecks"] > 0


def test_identical_rows_one_cluster_fast(gpu):
    X = np.tile(np.random.default_rng(1).standard_normal((1, 128)).astype(np.float32), (50000, 1))
    x = torch.from_numpy(X).cuda()
    _fit(x[:300], 0.14, 2)                                           # code objects loaded
    torch.cuda.synchronize()
    t = time.time()
    m = _fit(x, 0.14, 2)
    dt = time.time() - t
    assert m.n_clusters_ == 1 and np.all(m.labels_ == 0) and np.all(m.n_neighbors_ == 50000)
    assert len(m.core_sample_indices_) == 50000
    assert m.stats_["skipped_tiles"] > 0
    assert dt < 5.0, dt


def test_degenerate_inputs(gpu):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((5000, 512)).astype(np.float32)          # near-orthogonal: all noise
    m = _fit(X, 0.14, 2)
    assert np.all(m.labels_ == -1) and np.all(m.n_neighbors_ == 1) and m.n_clusters_ == 0
    m = _fit(X[:3000, :64], 2.0, 5)                                  # eps >= 2: one cluster
    assert np.all(m.labels_ == 0) and m.n_clusters_ == 1 and np.all(m.n_neighbors_ == 3000)
    for ms, want in ((1, 0), (2, -1)):                               # one row
        m = _fit(X[:1, :16], 0.14, ms)
        assert m.labels_.tolist() == [want]
    Z = np.concatenate([_blobs(5, 2000, 16, 8, 0.15), np.zeros((7, 16), np.float32)])   # zero rows
    Z = Z[np.random.default_rng(6).permutation(len(Z))]
    for eps, ms in ((0.14, 2), (0.14, 1), (1.05, 3)):
        _check_against_oracle(Z, eps, ms)


def test_large_sampled_properties(gpu):
    N, D = 100000, 128
    X = _blobs(11, N, D, K=200, spread=0.25)
    eps, ms = 0.14, 5
    m = _fit(torch.from_numpy(X).cuda(), eps, ms)
    lab, cnt = m.labels_, m.n_neighbors_
    core = np.zeros(N, bool)
    core[m.core_sample_indices_] = True
    assert np.array_equal(core, cnt >= ms)
    X64 = X.astype(np.float64)
    inv = inv_norms(X64)
    rows = np.random.default_rng(0).choice(N, 512, replace=False)
    d = np.clip(1.0 - (X64[rows] @ X64.T) * inv[rows, None] * inv[None, :], 0.0, 2.0)
    d[np.arange(512), rows] = 0.0
    nb = d <= eps
    assert np.array_equal(cnt[rows], nb.sum(1))
    n_border = 0
    for i, r in enumerate(rows):
        cn = np.flatnonzero(nb[i] & core)
        if core[r]:
            assert np.all(lab[cn] == lab[r])
        elif len(cn):
            assert lab[r] == lab[cn].min()
            n_border += 1
        else:
            assert lab[r] == -1
    assert core[rows].any() and (~core[rows]).any()


def test_deterministic_and_input_forms(gpu):
    X = _blobs(21, 6000, 100, 20, 0.3)
    a = _fit(X, 0.14, 3)
    b = _fit(torch.from_numpy(X), 0.14, 3)
    x = torch.from_numpy(X).cuda()
    c = _fit(x, 0.14, 3)
    d = _fit(x, 0.14, 3)
    for m in (b, c, d):
        assert np.array_equal(m.labels_, a.labels_)
        assert np.array_equal(m.core_sample_indices_, a.core_sample_indices_)
        assert np.array_equal(m.n_neighbors_, a.n_neighbors_)
    # a strided device view (row stride > D) is read in place
    wide = torch.zeros(6000, 128, device="cuda")
    wide[:, :100] = x
    e = _fit(wide[:, :100], 0.14, 3)
    assert np.array_equal(e.labels_, a.labels_)


def test_fit_cluster_end_to_end(gpu):
    from video_similarity_search_amd.clustering import fit_cluster
    X = _blobs(31, 4000, 128, 10, 0.3)
    out = fit_cluster(torch.from_numpy(X).cuda(), 'DBSCAN')
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.shape == (4000,)
    assert np.array_equal(out, dbscan_fp64(X, 0.14, 2)[0])
