"""GPU: OPTICS (cosine, cluster_method='dbscan') on the device (csrc/optics.hip) against the sklearn goldens and the float64 oracle
(tests/optics_cpu_kernels.py).
  G1  golden exact-order cases: labels equal sklearn's, ordering / predecessor equal the float64 walk's, values within (Dp + 8) 2^-24
  G2  two fits are bit-equal; a labels-only call gives the same labels
  G3  replay check where fp32 cannot fix the order (large D, a cluster beyond one workgroup, many two-row clusters, a zero row and exact
      duplicates): a float64 checker follows the DEVICE's ordering and verifies every pick and every reachability within
      tol = 2 (Dp + 8) 2^-24
  G4  the host cut of the device's plot at max_eps gives the device's labels; OPTICS(eps < max_eps) is the host cut of the full fit
  G5  fit_cluster(device tensor, 'OPTICS', max_eps=...)"""
import numpy as np
import pytest
import torch

from optics_cpu_kernels import core_distances, fp64_distances, optics_fp64
from test_optics_cpu import golden_cases, oracle

pytestmark = pytest.mark.gpu

EXACT = [c for c in golden_cases() if c["name"].startswith("exact_")]
U = 2.0 ** -24


def _dp(X):
    return (X.shape[1] + 7) // 8 * 8


_FITS = {}


def _fit(name, X, max_eps, ms):
    """one device fit per case, shared by the tests (read-only)"""
    if name not in _FITS:
        from video_similarity_search_amd.clustering.optics import OPTICS
        _FITS[name] = OPTICS(min_samples=ms, max_eps=max_eps).fit(torch.from_numpy(X).cuda())
    return _FITS[name]


def _fit_case(c):
    return _fit(c["name"], c["X"], c["max_eps"], c["min_samples"])


def _close(a, b, tol):
    fin = np.isfinite(b)
    return np.array_equal(np.isfinite(a), fin) and (not fin.any() or np.abs(a[fin].astype(np.float64) - b[fin]).max() <= tol)


# ---------------------------------------------------------------------------------------------------------------- G1

@pytest.mark.parametrize("case", EXACT, ids=lambda c: c["name"])
def test_g1_golden_exact_order(gpu, case):
    m = _fit_case(case)
    o = oracle(case)
    tol = (_dp(case["X"]) + 8) * U
    assert np.array_equal(m.labels_, case["sk_labels"])
    assert np.array_equal(np.isfinite(m.core_distances_), o["is_core"])
    assert np.array_equal(m.ordering_, case["ordering"])
    assert np.array_equal(m.predecessor_, case["predecessor"])
    assert _close(m.reachability_, case["reachability"], tol)
    assert _close(m.core_distances_, case["sk_core_distances"], tol)
    assert m.n_clusters_ == o["n_clusters"]
    assert m.stats_["walk_steps"] == np.bincount(o["labels"][o["labels"] >= 0]).max() and m.stats_["host_loop_clusters"] == 0


# ---------------------------------------------------------------------------------------------------------------- G1 at the scan's sizes

SCAN_D, SCAN_EPS, SCAN_MS = 16, 0.05, 3
# N -> seed: the first seed from N on whose float64 walk has gap >= 4 (Dp + 8) 2^-24 (the goldens' condition, asserted below) and,
# from N = 63 on, noise rows, two or more clusters and a border row, so that op_offsets places blocks of 1, of a cluster's size and of 0 rows
SCAN_SEEDS = {2: 2, 63: 65, 64: 88, 65: 71, 1023: 1043, 1024: 1025, 1025: 1058}


def _groups(seed, N):
    """N rows around far-apart centres: up to 12 groups of 3 .. 6 rows (clusters at min_samples = 3), the rest single rows and pairs (noise).
    Few clusters, so that a seed exists at every N whose walk never compares two values an ulp apart."""
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.integers(3, 7, min(12, N // 5))]
    while sum(sizes) < N:
        sizes.append(min(int(rng.integers(1, 3)), N - sum(sizes)))
    cen = rng.standard_normal((len(sizes), SCAN_D))
    X = np.repeat(cen, sizes, axis=0) + 0.1 * rng.uniform(0.5, 2.0, (N, 1)) * rng.standard_normal((N, SCAN_D))
    return X[rng.permutation(N)].astype(np.float32)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1023, 1024, 1025])
def test_g1_exact_order_at_the_scan_sizes(gpu, N):
    """the one-workgroup scan of op_offsets (1024 threads, runs of ceil(N / 1024) rows) with a partly filled last wave, empty trailing runs
    and runs of 1 next to runs of 2; G1's comparison against the float64 walk"""
    from video_similarity_search_amd.clustering.optics import OPTICS
    if N == 1:                                                                # min_samples <= N is a rule of the call: no launch
        with pytest.raises(ValueError, match="no greater than the number of samples"):
            OPTICS(min_samples=2, max_eps=SCAN_EPS).fit(torch.zeros(1, SCAN_D, device="cuda") + 1)
        return
    ms = min(SCAN_MS, N)
    X = _groups(SCAN_SEEDS[N], N)
    o = optics_fp64(X, SCAN_EPS, ms, want_gap=True)
    tol = (_dp(X) + 8) * U
    assert o["gap"] >= 4 * tol
    if N >= 63:
        assert (o["labels"] < 0).any() and o["n_clusters"] >= 2 and ((o["labels"] >= 0) & ~o["is_core"]).any()
    m = OPTICS(min_samples=ms, max_eps=SCAN_EPS).fit(torch.from_numpy(X).cuda())
    assert np.array_equal(m.labels_, o["labels"])
    assert np.array_equal(np.isfinite(m.core_distances_), o["is_core"])
    assert np.array_equal(m.ordering_, o["ordering"])
    assert np.array_equal(m.predecessor_, o["predecessor"])
    assert _close(m.reachability_, o["reachability"], tol)
    assert _close(m.core_distances_, o["core_distances"], tol)
    assert m.n_clusters_ == o["n_clusters"]


# ---------------------------------------------------------------------------------------------------------------- G3 data

def _scrub(X, max_eps, margin, fill):
    """replace every row that has a pair within `margin` of max_eps by a far-away row, until none is left"""
    for _ in range(20):
        d = fp64_distances(X)
        np.fill_diagonal(d, 2.0)
        bad = np.flatnonzero((np.abs(d - max_eps) < margin).any(axis=1))
        if not len(bad):
            return X
        X[bad] = fill(len(bad))
    raise AssertionError("pairs at max_eps remain")


def _case_a():
    """N = 1500, D = 200: one blob of > 1100 rows (every pair of its body a neighbour; a halo of rows around max_eps), forty blobs of
    3-12 rows, 60 uniform outliers"""
    rng = np.random.default_rng(22)
    N, D, eps = 1500, 200, 0.14
    sizes = rng.integers(3, 13, 40)
    big = N - 60 - int(sizes.sum())
    assert big > 1100
    rows = []
    c = rng.standard_normal(D)
    scale = np.full(big, 0.25)
    scale[:16] = 0.25 * rng.uniform(1.8, 2.4, 16)                            # the halo: distances to the body on both sides of max_eps
    rows.append(c + scale[:, None] * rng.standard_normal((big, D)))
    for s in sizes:
        c = rng.standard_normal(D)
        rows.append(c + 0.25 * rng.uniform(0.8, 2.2, (s, 1)) * rng.standard_normal((s, D)))
    rows.append(rng.uniform(-1, 1, (60, D)))
    X = np.concatenate(rows).astype(np.float32)[rng.permutation(N)]
    return X, eps, 5, lambda n: rng.uniform(-1, 1, (n, D)).astype(np.float32)


def _case_b():
    """N = 700, D = 24: 300 tight pairs and 100 singles; min_samples = 2: many clusters, two walk steps each"""
    rng = np.random.default_rng(12)
    D = 24
    u = rng.standard_normal((300, D))
    X = np.concatenate([u, u + 0.02 * rng.standard_normal((300, D)), rng.standard_normal((100, D))]).astype(np.float32)
    return X[rng.permutation(700)], 0.05, 2, lambda n: rng.standard_normal((n, D)).astype(np.float32)


def _case_c():
    """N = 300, D = 17: a zero row and 20 exact duplicates of other rows"""
    rng = np.random.default_rng(13)
    D = 17
    cen = rng.standard_normal((4, D))
    X = (cen[rng.integers(0, 4, 300)] + 0.45 * rng.standard_normal((300, D))).astype(np.float32)
    src, dst = rng.permutation(300)[:40].reshape(2, 20)
    X[dst] = X[src]
    X[7] = 0.0
    return X, 0.1, 3, lambda n: (3.0 * rng.standard_normal((n, D))).astype(np.float32)


_REPLAY = {}


def _replay_case(name):
    """-> (X, max_eps, min_samples, tol): built once; no pair within max(1e-5, tol) of max_eps (asserted)"""
    if name not in _REPLAY:
        X, eps, ms, fill = {"a": _case_a, "b": _case_b, "c": _case_c}[name]()
        tol = 2 * (_dp(X) + 8) * U
        margin = max(1e-5, tol)
        X = _scrub(X, eps, margin, fill)
        d = fp64_distances(X)
        assert np.abs(d[~np.eye(len(X), dtype=bool)] - eps).min() >= margin
        _REPLAY[name] = (X, eps, ms, tol, d)
    return _REPLAY[name]


def _check_replay(X, d, eps, ms, tol, m):
    """follow the DEVICE's ordering in float64"""
    N = len(X)
    core, cd = core_distances(d, eps, ms)
    order, reach, pred = m.ordering_.astype(np.int64), m.reachability_.astype(np.float64), m.predecessor_
    assert sorted(order.tolist()) == list(range(N))
    pos = np.empty(N, np.int64)
    pos[order] = np.arange(N)
    assert np.array_equal(np.isfinite(m.core_distances_), core)
    assert _close(m.core_distances_, cd, tol)
    fin = np.flatnonzero(np.isfinite(reach))
    p = pred[fin]
    assert np.all(p >= 0) and np.all(pred[~np.isfinite(reach)] == -1)
    assert np.all(core[p]) and np.all(pos[p] < pos[fin]) and np.all(d[p, fin] <= eps)
    assert np.abs(reach[fin] - np.maximum(d[p, fin], cd[p])).max(initial=0.0) <= tol
    R = np.full(N, np.inf)
    done = np.zeros(N, bool)
    worst = 0.0
    for t in range(N):
        q = order[t]
        left = np.flatnonzero(~done)
        lo = R[left].min()
        if np.isinf(lo):
            assert q == left[0], (t, "all unprocessed rows are at +inf: the pick is the lowest of them")
        else:
            assert R[q] - lo <= tol, (t, R[q], lo)
            worst = max(worst, R[q] - lo)
        done[q] = True
        if core[q]:
            nb = np.flatnonzero(~done & (d[q] <= eps))
            R[nb] = np.minimum(R[nb], np.maximum(d[q, nb], cd[q]))
    assert _close(m.reachability_, R, tol)                                    # the device's minimum is the replay's, within tol
    return worst


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_g3_replay(gpu, name):
    X, eps, ms, tol, d = _replay_case(name)
    m = _fit("replay_" + name, X, eps, ms)
    o = optics_fp64(X, eps, ms)
    worst = _check_replay(X, d, eps, ms, tol, m)
    assert np.array_equal(m.labels_, o["labels"])
    assert m.n_clusters_ == o["n_clusters"]
    sizes = np.bincount(o["labels"][o["labels"] >= 0])
    st = m.stats_
    print("replay {}: {} clusters, largest {}, {} walk launches, {} host-loop clusters, worst pick margin {:.3g} (tol {:.3g})".format(
        name, o["n_clusters"], sizes.max(), st["walk_launches"], st["host_loop_clusters"], worst, tol))
    assert st["largest_cluster"] == sizes.max() and st["walk_steps"] == sizes.max()
    if name == "a":
        assert sizes.max() > 1100 and st["host_loop_clusters"] == 1 and st["walk_launches"] == 2 * sizes.max() + 1
        assert ((o["labels"] >= 0) & ~o["is_core"]).any()                     # border rows inside the walk
    if name == "b":
        assert o["n_clusters"] >= 250 and sizes.max() <= 4 and st["host_loop_clusters"] == 0 and st["walk_launches"] == 1
    if name == "c":
        assert not X[7].any() and o["labels"][7] == -1 and np.isinf(m.reachability_[7])
        dup = (fp64_distances(X) + np.eye(len(X)) < 1e-15).any(axis=1) & (np.abs(X).sum(axis=1) > 0)
        assert dup.sum() >= 20 and (o["labels"][dup] >= 0).any()


# ---------------------------------------------------------------------------------------------------------------- G2

@pytest.mark.parametrize("which", ["exact_d16_a", "replay_a"])
def test_g2_bit_equal_rerun_and_labels_only(gpu, which):
    from video_similarity_search_amd.clustering.optics import OPTICS, HipOpticsKernels
    if which == "replay_a":
        X, eps, ms = _replay_case("a")[:3]
    else:
        c = [c for c in EXACT if c["name"] == which][0]
        X, eps, ms = c["X"], c["max_eps"], c["min_samples"]
    a = _fit(which, X, eps, ms)
    b = OPTICS(min_samples=ms, max_eps=eps).fit(torch.from_numpy(X).cuda())
    for f in ("labels_", "ordering_", "predecessor_"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("reachability_", "core_distances_"):
        assert np.array_equal(getattr(a, f).view(np.int32), getattr(b, f).view(np.int32)), f
    k = HipOpticsKernels()
    labels, core, cd, reach, pred, order, ncl = k.optics(k.resident(X), eps, ms, walk=False)
    assert cd is None and reach is None and pred is None and order is None
    assert np.array_equal(labels, a.labels_) and np.array_equal(core, np.isfinite(a.core_distances_)) and ncl == a.n_clusters_
    assert k.last_stats["walk_launches"] == 0


# ---------------------------------------------------------------------------------------------------------------- G4

def test_g4_host_cut_of_the_device_plot_gives_the_device_labels(gpu):
    from video_similarity_search_amd.clustering.optics import OPTICS, cluster_optics_dbscan
    fits = [(_fit_case(c), c["max_eps"]) for c in EXACT]
    fits += [(_fit("replay_" + n, *_replay_case(n)[:3]), _replay_case(n)[1]) for n in ("a", "b", "c")]
    for m, eps in fits:
        cut = cluster_optics_dbscan(reachability=m.reachability_, core_distances=m.core_distances_, ordering=m.ordering_, eps=eps)
        assert np.array_equal(cut, m.labels_)
    c = EXACT[0]
    full = _fit_case(c)
    e = 0.6 * c["max_eps"]
    lo = OPTICS(min_samples=c["min_samples"], max_eps=c["max_eps"], eps=e).fit(c["X"])
    want = cluster_optics_dbscan(reachability=full.reachability_, core_distances=full.core_distances_, ordering=full.ordering_, eps=e)
    assert np.array_equal(lo.labels_, want) and not np.array_equal(lo.labels_, full.labels_)
    assert np.array_equal(lo.ordering_, full.ordering_)


# ---------------------------------------------------------------------------------------------------------------- G5

def test_g5_fit_cluster_wiring(gpu, capsys):
    from video_similarity_search_amd.clustering import fit_cluster
    c = EXACT[0]
    out = fit_cluster(torch.from_numpy(c["X"]).cuda(), 'OPTICS', max_eps=c["max_eps"], min_samples=c["min_samples"])
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, c["sk_labels"])
    n = len(set(c["sk_labels"].tolist()) - {-1})
    assert capsys.readouterr().out.splitlines() == ["Clustering with OPTICS...", str((len(c["X"]),)),
                                                    "Fitted {} clusters with OPTICS".format(n)]
    c = [c for c in golden_cases() if c["name"] == "plain_d24_ms3"][0]            # min_samples defaults to the reference's 3
    assert np.array_equal(fit_cluster(c["X"], 'OPTICS', max_eps=0.2), c["sk_labels"])
