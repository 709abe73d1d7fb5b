"""GPU: HDBSCAN (cosine) on the device (csrc/hdbscan.hip).  The entry points are called directly over the smallest shapes at which they
can go wrong (tails in both operands, padding to 8, more than one k-tile, more than one query and gallery tile) and over the component
layouts of a Boruvka run, against the float64 restatement (tests/hdbscan_cpu_kernels.py); then the driver on the sklearn goldens.
Harness: outputs start as NaN / -1, the workspace carries the 4096-byte guard tail of tests/test_bn_pool_gpu.py, every call runs twice
and the two results must be bit-equal.
Gates are derived, not measured.  u = 2^-24, b = 2 (Dp + 2) u: the bound csrc/dbscan.hip uses for an fp32 score of unit rows, doubled as
there.  A row's reported weight is within b of the float64 minimum over the foreign rows; the tree's sorted float64 weights are within b,
element by element, of the exact MST weights (MST bottleneck weights are 1-Lipschitz in the sup norm of the weights)."""
import numpy as np
import pytest
import torch

from hdbscan_cpu_kernels import (core_fp64, distances_fp64, hdbscan_tree_fp64, is_spanning_tree, mutual_reachability, prim_weights,
                                 same_partition)
from test_hdbscan_cpu import golden_cases

pytestmark = pytest.mark.gpu

GUARD = 4096
U = 2.0 ** -24


def band(D):
    return 2.0 * ((D + 7) // 8 * 8 + 2) * U


def _rows(seed, N, D):
    """clustered rows of arbitrary norm plus noise rows; a zero row from N = 127 on"""
    rng = np.random.default_rng(seed)
    K = max(2, N // 60)
    cen = rng.standard_normal((K, D))
    X = cen[rng.integers(0, K, N)] + 0.25 * rng.standard_normal((N, D))
    nn = N // 8
    X[:nn] = rng.standard_normal((nn, D))
    X *= rng.uniform(0.5, 3.0, (N, 1))
    X = X[rng.permutation(N)].astype(np.float32)
    if N >= 127:
        X[N // 3] = 0.0
    return X


class Device:
    """the three entry points on guarded buffers; every call twice, bit-equal"""

    def __init__(self, X, ms):
        from video_similarity_search_amd import _lib
        self._lib = _lib
        self.N, self.D, self.ms = X.shape[0], X.shape[1], ms
        self.x = torch.from_numpy(X).cuda()
        nbytes = int(_lib.load().slic_hdbscan_workspace_bytes(self.N, self.D, ms))
        assert nbytes > 0
        self.nbytes = nbytes
        self.pattern = (torch.arange(GUARD) % 251).to(torch.uint8).cuda()
        self.ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device="cuda")
        self.ws[nbytes:] = self.pattern

    def _call(self, name, *args):
        p = self._lib.ptr
        self._lib.call(name, *[p(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], self._lib.stream())
        torch.cuda.synchronize()
        assert torch.equal(self.ws[self.nbytes:], self.pattern), f"{name} wrote past its workspace of {self.nbytes} bytes"

    def core(self):
        outs = []
        for _ in range(2):
            c = torch.full((self.N,), float("nan"), dtype=torch.float64, device="cuda")
            self._call("slic_hdbscan_core", self.x, self.N, self.x.stride(0), self.D, self.ms, c, self.ws)
            outs.append(c)
        assert torch.equal(outs[0], outs[1])
        self.core_dev = outs[0]
        return outs[0].cpu().numpy()

    def round(self, comp, C):
        """-> (lo int32 [C], hi int32 [C], w float32 [C], row_w float32 [N], row_j int32 [N])"""
        dcomp = torch.from_numpy(np.ascontiguousarray(comp, dtype=np.int32)).cuda()
        outs = []
        for _ in range(2):
            oi = torch.full((C,), -7, dtype=torch.int32, device="cuda")
            oj = torch.full((C,), -7, dtype=torch.int32, device="cuda")
            ow = torch.full((C,), float("nan"), dtype=torch.float32, device="cuda")
            rb = torch.full((self.N,), -7, dtype=torch.int64, device="cuda")
            self._call("slic_hdbscan_round", self.ws, self.N, self.D, self.ms, dcomp, C, oi, oj, ow, rb)
            outs.append((oi, oj, ow, rb))
        for a, b in zip(*outs):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
        oi, oj, ow, rb = (t.cpu().numpy() for t in outs[0])
        rb = rb.view(np.uint64)
        row_w = (rb >> np.uint64(32)).astype(np.uint32).view(np.float32)
        row_j = (rb & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        return oi, oj, ow, row_w, row_j

    def weights(self, pairs):
        dp = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).cuda()
        outs = []
        for _ in range(2):
            o = torch.full((len(pairs),), float("nan"), dtype=torch.float64, device="cuda")
            self._call("slic_hdbscan_edge_weights", self.x, self.N, self.x.stride(0), self.D, self.ms, self.core_dev, dp, len(pairs), o, self.ws)
            outs.append(o)
        assert torch.equal(outs[0], outs[1])
        return outs[0].cpu().numpy()


def _check_round(dev, W, comp, C, b):
    """one round against the float64 weights W: per row, then the reduction per component (exact, from the rows' own values)"""
    N = len(W)
    oi, oj, ow, row_w, row_j = dev.round(comp, C)
    foreign = comp[:, None] != comp[None, :]
    want = np.where(foreign, W, np.inf).min(axis=1)
    has = np.isfinite(want)
    assert np.array_equal(row_j >= 0, has)
    r = np.flatnonzero(has)
    print("round: N = {}, C = {}, max |w - w64| = {:.3g} (b = {:.3g})".format(N, C, np.abs(row_w[r] - want[r]).max() if len(r) else 0.0, b))
    assert np.all(np.abs(row_w[r].astype(np.float64) - want[r]) <= b)
    assert np.all(foreign[r, row_j[r]])                                             # the mask
    assert np.all(np.abs(W[r, row_j[r]] - want[r]) <= 2 * b)                        # the row named carries that weight
    # per component: the least (w, lo, hi) of its rows' candidates, bit for bit
    lo, hi = np.minimum(r, row_j[r]), np.maximum(r, row_j[r])
    elo, ehi, ew = np.full(C, -1, np.int32), np.full(C, -1, np.int32), np.full(C, np.inf, np.float32)
    for t in np.lexsort((hi, lo, row_w[r]))[::-1].tolist():
        c = comp[r[t]]
        elo[c], ehi[c], ew[c] = lo[t], hi[t], row_w[r[t]]
    assert np.array_equal(oi, elo) and np.array_equal(oj, ehi) and np.array_equal(ow.view(np.int32), ew.view(np.int32))
    return oi, oj


CASES = [(N, D, ms) for N in (2, 127, 129, 300, 1000) for D in (3, 32, 40, 512) for ms in (1, 2, 5) if ms <= N]
# hd_tiles<NK> holds a row in NK = 4 ceil(Dp / 128) k-tiles: the D above reach NK = 4 and 16, these NK = 8 and 12
CASES += [(N, D, ms) for N in (129, 300) for D in (200, 320) for ms in (2, 5)]


@pytest.mark.parametrize("N,D,ms", CASES)
def test_entry_points_against_fp64(gpu, N, D, ms):
    from video_similarity_search_amd.clustering.hdbscan import boruvka_mst
    X = _rows(1000 * N + 10 * D + ms, N, D)
    b = band(D)
    d = distances_fp64(X)
    core = core_fp64(d, ms)
    W = mutual_reachability(d, core)
    dev = Device(X, ms)
    got = dev.core()
    print("core: max |core - core64| = {:.3g} (b = {:.3g})".format(np.abs(got - core).max(), b))
    assert np.all(np.abs(got - core) <= b)
    _check_round(dev, W, np.arange(N, dtype=np.int32), N, b)
    # the whole tree through the same entry points
    edges, w = boruvka_mst(N, lambda comp, C: dev.round(comp, C)[:2], dev.weights)
    assert is_spanning_tree(edges, N)
    assert np.all(edges[:, 0] < edges[:, 1])
    assert np.all(np.abs(w - W[edges[:, 0], edges[:, 1]]) <= b)                     # float64 weights of the device's own core distances
    exact = prim_weights(W)
    print("tree: max |sorted w - exact| = {:.3g} (b = {:.3g})".format(np.abs(np.sort(w) - exact).max(), b))
    assert np.all(np.abs(np.sort(w) - exact) <= b)
    assert np.all(np.diff(w) >= 0)                                                  # tree order


@pytest.mark.parametrize("layout", ["singletons", "interleaved", "all_but_one", "duplicates", "one_component"])
def test_component_layouts(gpu, layout):
    N, D, ms = 300, 40, 2
    X = _rows(77, N, D)
    comp = np.arange(N, dtype=np.int32)
    if layout == "interleaved":
        comp = (np.arange(N) % 2).astype(np.int32)
    elif layout == "all_but_one":
        comp = np.zeros(N, np.int32)
        comp[211] = 1
    elif layout == "duplicates":
        X[200] = X[5]
        X[131] = 2.5 * X[130]                                                       # the same direction: a duplicate for the metric
    elif layout == "one_component":
        comp = np.zeros(N, np.int32)
    C = int(comp.max()) + 1
    d = distances_fp64(X)
    W = mutual_reachability(d, core_fp64(d, ms))
    dev = Device(X, ms)
    dev.core()
    oi, oj = _check_round(dev, W, comp, C, band(D))
    if layout == "one_component":
        assert oi.tolist() == [-1] and oj.tolist() == [-1]
    if layout == "duplicates":
        assert (oi[5], oj[5]) == (5, 200) and (oi[130], oj[130]) == (130, 131)


def test_rejected_arguments(gpu):
    from video_similarity_search_amd import _lib
    X = _rows(3, 64, 16)
    dev = Device(X, 2)
    dev.core()
    comp = torch.zeros(64, dtype=torch.int32, device="cuda")
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    for C in (0, 65):
        with pytest.raises(_lib.SlicError):
            dev._call("slic_hdbscan_round", dev.ws, 64, 16, 2, comp, C, out, out, out.view(torch.float32), None)
    with pytest.raises(_lib.SlicError):
        dev._call("slic_hdbscan_core", dev.x, 64, 16, 16, 65, dev.core_dev, dev.ws)


def _fit(X, mcs, ms, method, single, eps):
    from video_similarity_search_amd.clustering.hdbscan import HDBSCAN
    return HDBSCAN(min_cluster_size=mcs, min_samples=ms, cluster_selection_method=method, allow_single_cluster=single,
                   cluster_selection_epsilon=eps).fit(X)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_driver_on_goldens(gpu, case):
    X, N = case["X"], len(case["X"])
    m = _fit(torch.from_numpy(X).cuda(), case["mcs"], case["ms"], case["method"], case["single"], case["eps"])
    assert m.labels_.dtype == np.int32 and m.probabilities_.dtype == np.float64
    assert m.mst_edges_.shape == (N - 1, 2) and m.mst_edges_.dtype == np.int32 and is_spanning_tree(m.mst_edges_, N)
    st = case["stable"]
    assert same_partition(m.labels_[st], case["labels"][st])
    pos = m.mst_weights_[m.mst_weights_ > 0]
    tol = 4 * band(X.shape[1]) / pos.min()
    print("probabilities: max |p - sklearn| on the mask = {:.3g} (4 b / h_min = {:.3g})".format(np.abs(m.probabilities_ - case["prob"])[st].max(), tol))
    assert np.all(np.abs(m.probabilities_ - case["prob"])[st] <= tol)
    # the host part alone: the oracle's tree function fed the device's own MST
    labels, prob = hdbscan_tree_fp64(m.mst_edges_, m.mst_weights_, N, case["mcs"], case["method"], case["single"], case["eps"])
    assert np.array_equal(labels, m.labels_)
    assert np.all(np.abs(prob - m.probabilities_) <= 1e-12)
    assert m.n_clusters_ == int(m.labels_.max()) + 1
    for cut, want in case["cuts"]:
        assert same_partition(m.dbscan_clustering(cut, case["mcs"]), want)
    assert m.stats_["rounds"] <= int(np.ceil(np.log2(N)))


def test_fit_cluster_end_to_end_and_input_forms(gpu, capsys):
    from video_similarity_search_amd.clustering import fit_cluster
    case = [c for c in golden_cases() if c["name"] == "a_mcs5_ms2"][0]
    X = case["X"]
    out = fit_cluster(torch.from_numpy(X).cuda(), 'HDBSCAN', min_cluster_size=5, min_samples=2)
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.shape == (len(X),)
    assert same_partition(out, case["labels"])
    n = int(out.max()) + 1
    assert capsys.readouterr().out.splitlines() == ["Clustering with HDBSCAN...", str((len(X),)), "Fitted {} clusters with HDBSCAN".format(n)]
    assert fit_cluster.last_model.n_clusters_ == n
    # a host array and a strided device view (row stride > D, read in place) give the same bits
    a = fit_cluster.last_model
    wide = torch.zeros(len(X), 48, device="cuda")
    wide[:, :32] = torch.from_numpy(X).cuda()
    for form in (X, wide[:, :32]):
        m = _fit(form, 5, 2, 'eom', False, 0.0)
        assert np.array_equal(m.labels_, a.labels_) and np.array_equal(m.mst_edges_, a.mst_edges_)
        assert np.array_equal(m.mst_weights_, a.mst_weights_) and np.array_equal(m.probabilities_, a.probabilities_)
