"""GPU: every driver that takes its scratch memory from `_lib.workspace` run on a buffer of EXACTLY the size its `*_workspace_bytes`
query (or, for MoCo, the Python expression) asks for — guarded on both sides, poisoned inside (tests/ws_guard.py).

The production allocator is a grow-only cache, so inside one pytest process a small shape runs on a buffer a larger case grew: a query
that is short by a row, a pad or a slice at the small shapes, or a kernel that reads a workspace slot nothing in the same call wrote,
stays invisible.  Every case here does the same five things:
  1. runs the driver under the guarded allocator with poison 0x00, then in a fresh one with poison 0xFF (NaN as float / double, -1 as int32);
  2. checks every guard byte after each run;
  3. asserts the request log holds the case's tag(s) and that every size equals what the query returns for those arguments (a driver
     that asked for no workspace fails the case);
  4. holds the outputs of the 0xFF run against the float64 oracle or golden of the driver's own test file, under that file's gate —
     oracles, data makers and gates are imported from there; where a gate is a literal inside an existing test body it is repeated
     here with the test's name beside it;
  5. asserts the two runs bit-equal wherever the suite already asserts run-to-run bit equality for the call (top-k, DBSCAN, OPTICS,
     agglomerative, metrics, t-SNE, clip transforms, MoCo, k-means labels and scores, the Winograd weight gradients); elsewhere both
     runs pass the gate of 4. and the case's docstring says why no more is claimed.
HDBSCAN, silhouette, NT-Xent, BatchNorm at entry level and the k-means entry points are called on exact guarded buffers by their own
test files and are not repeated here."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ws_guard import GUARD, GuardedWorkspace, guarded, run_both, spy_calls

pytestmark = pytest.mark.gpu


def _lib():
    from video_similarity_search_amd import _lib
    return _lib


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _same_bits(a, b):
    """bit equality of two arrays / tensors / scalars (NaN == NaN, -0.0 != 0.0)"""
    if torch.is_tensor(a):
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _only(ws, tag, want):
    """every request of the run went to `tag` and asked for `want` bytes; there was at least one"""
    assert ws.log, "the driver never asked for a workspace"
    assert set(ws.log) == {(tag, int(want))}, (ws.log, tag, int(want))


# =================================================================================================== the helper is not vacuous

def test_guard_catches_one_byte_either_side(gpu, monkeypatch):
    """no kernel of ours runs here: plain torch writes into the first guard byte behind a view and into the last byte before it make
    check() raise and name the tag and size; the view is exact, poisoned once, kept per (tag, size), fresh for another size"""
    lib = _lib()
    cuda = torch.device("cuda")
    for poison in (0x00, 0xFF):
        with guarded(monkeypatch, poison) as ws:
            v = lib.workspace(1000, cuda, "self")
            assert v.dtype == torch.uint8 and v.numel() == 1000 and bool((v == poison).all())
            whole = ws.allocation(v)
            assert whole.numel() == 1000 + 2 * GUARD and v.data_ptr() - whole.data_ptr() == GUARD and GUARD % 4096 == 0
            assert v.data_ptr() % 256 == 0                               # what SlicCarver's 256-byte carving rests on
            v[:] = 7
            again = lib.workspace(1000, cuda, "self")
            assert again.data_ptr() == v.data_ptr() and bool((again == 7).all())          # same key: same buffer, not poisoned again
            other = lib.workspace(1001, cuda, "self")
            assert other.data_ptr() != v.data_ptr() and other.numel() == 1001 and bool((other == poison).all())
            tiny = lib.workspace(1, cuda, "tiny")                         # no max(nbytes, 256)
            assert tiny.numel() == 1
            assert ws.log == [("self", 1000), ("self", 1000), ("self", 1001), ("tiny", 1)] and ws.sizes("self") == [1000, 1001]
            assert ws.lookup(v.data_ptr()) == ("self", 1000)
            ws.check()
            v[:] = poison
            v[-1] = 1                                                      # the last byte INSIDE: still fine
            v[0] = 1
            ws.check()
            whole[GUARD + 1000] ^= 0xFF                                    # one byte past the view
            with pytest.raises(AssertionError, match=r"'self' of 1000 bytes.*PAST"):
                ws.check()
            whole[GUARD + 1000] ^= 0xFF
            ws.check()
            whole[GUARD - 1] ^= 0xFF                                       # the last byte before it
            with pytest.raises(AssertionError, match=r"'self' of 1000 bytes.*BEFORE"):
                ws.check()
            whole[GUARD - 1] ^= 0xFF
            ws.check()
        assert lib.workspace is not ws                                     # the patch ended with the block
    assert lib.workspace(16, cuda, "self_after").numel() >= 256            # production behaviour untouched


# =================================================================================================== cosine top-k (tag `topk`)

def _gauss(seed, Nq, Ng, D):
    """the rows of test_topk_shapes_vs_oracle / test_topk_collect_equals_streaming: flat Gaussian, gallery row 3 zero"""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((Nq, D)).astype(np.float32)
    G = rng.standard_normal((Ng, D)).astype(np.float32)
    if Ng > 3:
        G[3] = 0.0
    return Q, G


def _tiled_gallery():
    """test_topk_collect_fallback_too_many_candidates / test_bf16_overflow_with_exact_duplicates: 64 distinct rows x 4096 copies"""
    rng = np.random.default_rng(3)
    base = rng.standard_normal((64, 64)).astype(np.float32)
    return rng.standard_normal((200, 64)).astype(np.float32), np.tile(base, (4096, 1)), base


def _cosine_two_runs(monkeypatch, Q, G, k, precision="fp32"):
    """steps 1, 2, 3 and 5 of a cosine_topk case -> (idx, dist, info) of the 0xFF run"""
    from video_similarity_search_amd.evaluate import cosine_topk
    lib = _lib().load()
    Nq, Ng, Dp = len(Q), len(Q) if G is None else len(G), (Q.shape[1] + 7) // 8 * 8

    def run():
        info = {}
        idx, dist = cosine_topk(Q, G, k=k, precision=precision, info=info)
        return idx.cpu().numpy(), dist.cpu().numpy(), info

    want = (lib.slic_cosine_topk_bf16_workspace_bytes(Nq, Ng, Dp, k) if precision == "bf16"
            else lib.slic_cosine_topk_workspace_bytes(Nq, Ng, k))
    (a, wa), (b, wb) = run_both(monkeypatch, run)
    for ws in (wa, wb):
        _only(ws, "topk", want)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and a[2] == b[2]
    print("cosine top-k", (Nq, Ng, Q.shape[1], k), precision, "workspace", int(want), "bytes, info", b[2])
    return b


STREAM_SHAPES = [(1, 50, 8, 50), (129, 1000, 128, 1), (33, 257, 40, 7),
                 (100, 5000, 512, 88),          # short pending columns; slices * k at the merge limit
                 (130, 700, 1024, 3)]           # the D > 512 kernel


@pytest.mark.parametrize("Nq,Ng,D,k", STREAM_SHAPES)
def test_cosine_topk_streaming(gpu, monkeypatch, Nq, Ng, D, k):
    from test_retrieval_nce_gpu import _topk_plan
    from test_topk_bf16_gpu import _vs_oracle
    assert not _topk_plan(Nq, Ng, (D + 7) // 8 * 8, k)["collect"]
    Q, G = _gauss(Nq + Ng, Nq, Ng, D)
    idx, dist, _ = _cosine_two_runs(monkeypatch, Q, G, k)
    _vs_oracle(Q, G, idx, dist, k, np.random.default_rng(1))


def test_cosine_topk_streaming_self_search(gpu, monkeypatch):
    from test_topk_bf16_gpu import _vs_oracle
    X = np.random.default_rng(300 + 40).standard_normal((300, 40)).astype(np.float32)
    idx, dist, _ = _cosine_two_runs(monkeypatch, X, None, 7)
    assert not np.any(idx == np.arange(300)[:, None])
    _vs_oracle(X, X, idx, dist, 7, np.random.default_rng(1), self_search=True)


@pytest.mark.parametrize("Nq,Ng,D,k", [(5, 32768, 64, 20), (257, 33000, 128, 1), (128, 40000, 512, 88)])
def test_cosine_topk_collect(gpu, monkeypatch, Nq, Ng, D, k):
    """SLIC_TOPK_COLLECT=1 (as test_retrieval_nce_gpu._topk_env sets it): the collect arrays and, behind them, the streaming arrays of
    the fallback are carved from one buffer"""
    from test_retrieval_nce_gpu import _topk_plan
    from test_topk_bf16_gpu import _vs_oracle
    monkeypatch.setenv("SLIC_TOPK_COLLECT", "1")
    assert _topk_plan(Nq, Ng, D, k)["collect"]
    Q, G = _gauss(Nq + Ng + k, Nq, Ng, D)
    idx, dist, _ = _cosine_two_runs(monkeypatch, Q, G, k)
    _vs_oracle(Q, G, idx, dist, k, np.random.default_rng(1))


def test_cosine_topk_collect_every_query_falls_back(gpu, monkeypatch):
    """the gallery of test_topk_collect_fallback_too_many_candidates: the candidate slots overflow for every query, so the collect
    arrays and the streaming arrays are both live in the one buffer; that test's gate: the nearest distinct row's copies, lowest index
    first"""
    from oracle import retrieval as orr
    from test_retrieval_nce_gpu import _topk_plan
    monkeypatch.setenv("SLIC_TOPK_COLLECT", "1")
    Q, G, base = _tiled_gallery()
    k = 50
    pl = _topk_plan(200, G.shape[0], 64, k)
    assert pl["collect"] and pl["cap"] < 4096
    idx, dist, _ = _cosine_two_runs(monkeypatch, Q, G, k)
    best = np.argmin(orr.cosine_distances(Q.astype(np.float64), base.astype(np.float64)), axis=1)
    assert np.array_equal(idx, best[:, None] + 64 * np.arange(k)[None, :])


def test_cosine_topk_bf16(gpu, monkeypatch):
    from test_topk_bf16_gpu import _vs_oracle
    monkeypatch.setenv("SLIC_TOPK_BF16", "1")
    Nq, Ng, D, k = 5, 32768, 64, 20
    Q, G = _gauss(Nq + Ng + k, Nq, Ng, D)
    idx, dist, info = _cosine_two_runs(monkeypatch, Q, G, k, precision="bf16")
    assert info["path"] == "bf16"
    _vs_oracle(Q, G, idx, dist, k, np.random.default_rng(1))
    assert (np.diff(dist, axis=1) >= 0).all()


def test_cosine_topk_bf16_every_query_overflows(gpu, monkeypatch):
    """test_bf16_overflow_with_exact_duplicates: all 200 queries overflow their candidate slots and are redone by the streaming kernels"""
    from oracle import retrieval as orr
    monkeypatch.setenv("SLIC_TOPK_BF16", "1")
    Q, G, base = _tiled_gallery()
    k = 50
    idx, dist, info = _cosine_two_runs(monkeypatch, Q, G, k, precision="bf16")
    assert info["path"] == "bf16" and info["overflow_queries"] == 200 and info["fallback_queries"] == 200
    best = np.argmin(orr.cosine_distances(Q.astype(np.float64), base.astype(np.float64)), axis=1)
    assert np.array_equal(idx, best[:, None] + 64 * np.arange(k)[None, :])


# =================================================================================================== euclidean top-k (tag `topk`)

@pytest.mark.parametrize("Nq,Ng,D,k,collect", [(1, 50, 8, 50, False),           # the searched list k + EU_MARGIN is clipped to Ng
                                               (33, 257, 40, 7, False),          # D % 8 != 0: centred padded copies in the workspace
                                               (100, 5000, 512, 88, False),
                                               (5, 32768, 64, 20, True)])
def test_euclidean_topk(gpu, monkeypatch, Nq, Ng, D, k, collect):
    from test_topk_euclidean_gpu import _check_vs_oracle, _oracle
    from video_similarity_search_amd.evaluate import euclidean_topk
    lib = _lib().load()
    if collect:
        monkeypatch.setenv("SLIC_TOPK_COLLECT", "1")
    Q, G = _gauss(Nq + Ng + 1, Nq, Ng, D)

    def run():
        idx, dist = euclidean_topk(Q, G, k=k)
        return idx.cpu().numpy(), dist.cpu().numpy()

    want = lib.slic_euclidean_topk_workspace_bytes(Nq, Ng, D, k)
    (a, wa), (b, wb) = run_both(monkeypatch, run)
    for ws in (wa, wb):
        _only(ws, "topk", want)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    _check_vs_oracle(b[0], b[1], *_oracle(Q, G, k))


# =================================================================================================== DBSCAN (tag `dbscan`)

def _dbscan_case(monkeypatch, X, eps, ms):
    from dbscan_cpu_kernels import dbscan_fp64
    from video_similarity_search_amd.clustering.dbscan import DBSCAN
    lib = _lib().load()
    N, D = X.shape
    labels, core, counts, ncl = dbscan_fp64(X, eps, ms)

    def run():
        m = DBSCAN(eps=eps, min_samples=ms).fit(torch.from_numpy(X).cuda())
        return m.labels_, m.n_neighbors_, m.core_sample_indices_, m.n_clusters_

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    for ws in (wa, wb):
        _only(ws, "dbscan", lib.slic_dbscan_cosine_workspace_bytes(N, D))
    assert all(_same_bits(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    # test_dbscan_gpu._check_against_oracle's comparison
    assert np.array_equal(b[1], counts) and np.array_equal(b[2], np.flatnonzero(core)) and np.array_equal(b[0], labels) and b[3] == ncl
    return labels, core, counts, ncl


@pytest.mark.parametrize("N", [1, 2, 65, 1025, 2049])
def test_dbscan_scan_sizes(gpu, monkeypatch, N):
    from test_dbscan_gpu import SCAN_SEEDS, _blobs
    D, eps, ms = 8, 0.05, 3
    X = _blobs(SCAN_SEEDS[N], N, D, K=max(4, N // 400), spread=0.15)
    labels, core, counts, _ = _dbscan_case(monkeypatch, X, eps, ms)
    if N >= 63:
        assert core.any() and ((counts >= 2) & ~core).any() and (labels == -1).any()


@pytest.mark.parametrize("N,D,eps,ms", [(3000, 100, 0.14, 5),         # the padding to 8
                                        (3000, 200, 0.3, 3)])         # the 8-k-tile instantiation
def test_dbscan_padding_and_k_tiles(gpu, monkeypatch, N, D, eps, ms):
    from test_dbscan_gpu import _blobs
    X = _blobs(N + D, N, D, K=max(4, N // 400), spread=0.3)
    labels, _, _, ncl = _dbscan_case(monkeypatch, X, eps, ms)
    assert ncl > 1 and (labels == -1).any()


# =================================================================================================== OPTICS (tag `optics`)

def _optics_two_runs(monkeypatch, X, eps, ms):
    from video_similarity_search_amd.clustering.optics import OPTICS
    lib = _lib().load()
    N, D = X.shape

    def run():
        return OPTICS(min_samples=ms, max_eps=eps).fit(torch.from_numpy(X).cuda())

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    for ws in (wa, wb):
        _only(ws, "optics", lib.slic_optics_cosine_workspace_bytes(N, D, ms))
    for f in ("labels_", "ordering_", "predecessor_", "reachability_", "core_distances_"):           # test_g2's fields
        assert _same_bits(getattr(a, f), getattr(b, f)), f
    assert a.n_clusters_ == b.n_clusters_
    return b


@pytest.mark.parametrize("N", [2, 65, 1025])
def test_optics_scan_sizes(gpu, monkeypatch, N):
    """test_g1_exact_order_at_the_scan_sizes on exact buffers"""
    from optics_cpu_kernels import optics_fp64
    from test_optics_gpu import SCAN_EPS, SCAN_MS, SCAN_SEEDS, U, _close, _dp, _groups
    ms = min(SCAN_MS, N)
    X = _groups(SCAN_SEEDS[N], N)
    o = optics_fp64(X, SCAN_EPS, ms, want_gap=True)
    tol = (_dp(X) + 8) * U
    assert o["gap"] >= 4 * tol
    if N >= 63:
        assert (o["labels"] < 0).any() and o["n_clusters"] >= 2 and ((o["labels"] >= 0) & ~o["is_core"]).any()
    m = _optics_two_runs(monkeypatch, X, SCAN_EPS, ms)
    assert np.array_equal(m.labels_, o["labels"])
    assert np.array_equal(np.isfinite(m.core_distances_), o["is_core"])
    assert np.array_equal(m.ordering_, o["ordering"])
    assert np.array_equal(m.predecessor_, o["predecessor"])
    assert _close(m.reachability_, o["reachability"], tol)
    assert _close(m.core_distances_, o["core_distances"], tol)
    assert m.n_clusters_ == o["n_clusters"]


def test_optics_cluster_beyond_one_workgroup(gpu, monkeypatch):
    """replay case "a" of test_g3_replay (N = 1500, D = 200): the only G3 case whose largest cluster (> 1100 rows) exceeds one workgroup"""
    from optics_cpu_kernels import optics_fp64
    from test_optics_gpu import _check_replay, _replay_case
    X, eps, ms, tol, d = _replay_case("a")
    o = optics_fp64(X, eps, ms)
    sizes = np.bincount(o["labels"][o["labels"] >= 0])
    assert sizes.max() > 1100 and ((o["labels"] >= 0) & ~o["is_core"]).any()
    m = _optics_two_runs(monkeypatch, X, eps, ms)
    _check_replay(X, d, eps, ms, tol, m)
    assert np.array_equal(m.labels_, o["labels"]) and m.n_clusters_ == o["n_clusters"]
    assert m.stats_["largest_cluster"] == sizes.max() and m.stats_["host_loop_clusters"] == 1


# =================================================================================================== agglomerative (own buffer + tag `agglo_topk`)

def _guarded_agglo(poison):
    """HipAggloKernels with the state of a run on a guarded exact buffer (start allocates with torch.empty itself, not through
    _lib.workspace) — in the manner of test_hdbscan_gpu.Device; the top-k workspace of every round comes through the patched allocator"""
    from video_similarity_search_amd.clustering.agglomerative import HipAggloKernels
    lib = _lib()

    class Guarded(HipAggloKernels):
        def start(self, rows):
            N, D = rows.shape
            nbytes = int(lib.load().slic_agglo_workspace_bytes(N, D))
            assert nbytes > 0
            self.state = GuardedWorkspace(poison)
            self.N, self.D, self.A, self.Q = N, D, N, N
            self.ws = self.state(nbytes, rows.device, "agglo")
            self.rec = (ctypes.c_int64 * 5)()
            self.search_ns = 0
            self.topk_want = []
            bad = ctypes.c_int32(0)
            lib.call("slic_agglo_start", lib.ptr(rows), N, rows.stride(0), D, lib.ptr(self.ws), ctypes.byref(bad), lib.stream())
            self.state.check()
            return int(bad.value)

        def round(self, threshold):
            self.topk_want.append(("agglo_topk", int(lib.load().slic_cosine_topk_workspace_bytes(self.Q, self.A, 2))))
            return super().round(threshold)

    return Guarded()


def _agglo_cases():
    from test_agglomerative_gpu import ORACLE_CASES
    # 1025 rows: two scan blocks of 1024 ids; the seed is the first from 0 on whose float64 run has oracle_gap >= GAP (asserted below)
    return list(ORACLE_CASES[:5]) + [(1025, 16, 0.2, (AGGLO_1025_SEED, 6, 0.4, 4, 0.4))]


AGGLO_1025_SEED = 0


@pytest.mark.parametrize("i", range(6))
def test_agglomerative(gpu, monkeypatch, i):
    from test_agglomerative_gpu import GAP, oracle
    from video_similarity_search_amd.clustering import AgglomerativeClustering
    case = _agglo_cases()[i]
    X, labels, gap = oracle(case)
    print("case", case[:3], "oracle gap", gap, "clusters", labels.max() + 1)
    assert gap >= GAP                                            # decidable in fp32: asserted on the CPU first
    if case[0] == 1025:
        assert 1 < labels.max() + 1 < 1025 / 1.5 and np.bincount(labels).max() > 2          # test_cases_are_not_trivial's rule
    runs = []
    for poison in (0x00, 0xFF):
        k = _guarded_agglo(poison)
        with guarded(monkeypatch, poison) as ws:
            m = AgglomerativeClustering(distance_threshold=case[2], kernels=k).fit(torch.tensor(X).cuda())
            ws.check()
        k.state.check()
        assert m.rounds_ >= 1 and ws.log == k.topk_want, (ws.log, k.topk_want)
        runs.append(m)
    a, b = runs
    assert a.labels_.tobytes() == b.labels_.tobytes() and (a.rounds_, a.n_query_rows_) == (b.rounds_, b.n_query_rows_)
    assert np.array_equal(b.labels_, labels) and b.n_clusters_ == labels.max() + 1


# =================================================================================================== NMI / AMI (tag `cluster_metrics`)

def _metrics_case(monkeypatch, lt, lp, max_cells=None):
    from cluster_metrics_cpu_kernels import cluster_metrics_fp64
    from test_cluster_metrics_cpu import GATE, KEYS
    from video_similarity_search_amd.clustering import cluster_scores
    lib = _lib().load()
    N = len(lt)
    cells = min(N * N, (1 << 26) if max_cells is None else max_cells)

    def run():
        return cluster_scores(torch.from_numpy(lt).cuda(), torch.from_numpy(lp).cuda(), max_cells=max_cells)

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    for ws in (wa, wb):
        _only(ws, "cluster_metrics", lib.slic_cluster_metrics_workspace_bytes(N, cells))
    assert a == b                                                                       # test_bit_identical_across_runs_and_input_forms
    ref = cluster_metrics_fp64(lt, lp)
    got = np.array([b[k] for k in KEYS])
    print("N", N, "max |device - provider| =", np.abs(got - ref[:6]).max(), "gate", GATE)
    assert (b["n_classes"], b["n_clusters"]) == (int(ref[6]), int(ref[7])) and ref[8] == 0
    assert (b["n_classes"], b["n_clusters"]) == (len(np.unique(lt)), len(np.unique(lp)))
    assert np.abs(got - ref[:6]).max() <= GATE, (got, ref)


@pytest.mark.parametrize("N", [1, 1025, 4097])
def test_cluster_metrics_scan_sizes(gpu, monkeypatch, N):
    rng = np.random.default_rng(1000 + N)                                                # test_scan_sizes_against_the_provider's labels
    lt = rng.integers(-3, 9, N).astype(np.int32)
    lp = np.where(rng.random(N) < 0.5, lt * 3 + rng.integers(0, 3, N), rng.integers(-40, 40, N)).astype(np.int32)
    _metrics_case(monkeypatch, lt, lp)


def test_cluster_metrics_bounded_table(gpu, monkeypatch):
    rng = np.random.default_rng(9)                                                       # test_max_cells_bounds_the_table's labels
    lt, lp = rng.integers(0, 40, 20000).astype(np.int32), rng.integers(0, 100, 20000).astype(np.int32)
    assert len(np.unique(lt)) * len(np.unique(lp)) == 4000                               # exactly the bound
    _metrics_case(monkeypatch, lt, lp, max_cells=4000)


# =================================================================================================== t-SNE (tag `tsne`), PCA (tag `pca_cs`)

@pytest.mark.parametrize("N", [2, 65, 257])
def test_tsne_symmetrize_and_step(gpu, monkeypatch, N):
    """symmetrize under test_symmetrize's derived bound; one step under test_forces' bound, 4 x the float32 restatement's distance from
    float64 in ulp of the row's absolute-term sum (stored for N = 65 and 257 at scale 1, exaggeration 12).  N = 2 has no stored figure:
    the restatement is run here on the same input as make_goldens_tsne.py runs it; with one pair a component is two products of at most
    8 fp32 roundings each (difference, square, sum, 1 +, reciprocal, e P w or w w, times the difference, over Z), 4 ulp of 2^-23 for the
    larger one, and one more for the subtraction, so the bound is the larger of 4 x the restatement's figure and 5 ulp"""
    import tsne_ref as R
    from test_tsne_gpu import Z, dev, one_step
    from tsne_cpu_kernels import NumpyTsneKernels
    from video_similarity_search_amd.manifold import HipTsneKernels
    lib = _lib().load()
    e = 12.0
    if N == 2:
        Pc = np.array([[0.0, 1.0], [1.0, 0.0]], dtype=np.float32)
        Ph = R.joint(Pc).astype(np.float32)
        Y = np.random.RandomState(7).standard_normal((2, 2)).astype(np.float32)
    else:
        d2 = R.sqdist64(R.blobs(N, 8, 300 + N, outlier=False)).astype(np.float32)
        Pc = R.cond_p64(d2, min(30.0, (N - 1) / 3.0)).astype(np.float32)
        Ph = R.joint_input((N,))
        Y = R.embedding(N, 1.0, 7)
    g64, Z64, kl64, S = R.forces64(Ph, Y, e)
    if N == 2:
        g32 = NumpyTsneKernels().forces(Ph, Y, e, True)[0]
        bound = max(4.0 * float((np.abs(g32 - g64) / S).max() / R.ULP32), 5.0)
    else:
        bound = 4.0 * float(Z[R.force_key((N, 1.0, e)) + "_r32_ulp"])

    def run():
        K = HipTsneKernels()
        J = K.symmetrize(dev(Pc.copy())).cpu().numpy()
        return (J,) + one_step(K, dev(Ph), Y, np.zeros_like(Y), np.ones_like(Y), e, 0.0, 0.0)

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    for ws in (wa, wb):
        _only(ws, "tsne", lib.slic_tsne_workspace_bytes(N))
        assert len(ws.log) >= 2                                                           # symmetrize and the step
    assert all(_same_bits(x, y) for x, y in zip(a, b))                                   # test_twenty_steps: two runs, the same bits
    J, _, _, _, grad, rec = b
    ref = R.joint(Pc.astype(np.float64))
    print("N", N, "symmetrize: max |J - ref|", np.abs(J - ref).max(), "bound", 2.0 ** -24 * ref.max() + R.EPS)
    assert np.array_equal(J, J.T) and (np.diag(J) == 0).all()
    assert np.abs(J - ref).max() <= 2.0 ** -24 * ref.max() + R.EPS
    assert np.isfinite(grad).all() and np.isfinite(rec).all()
    ulp = (np.abs(grad - g64) / S).max() / R.ULP32
    print("N", N, "gradient error", ulp, "ulp; bound", bound, "ulp; Z off by", abs(rec[0] / Z64 - 1), "KL off by", abs(rec[1] / kl64 - 1))
    assert ulp <= bound
    assert abs(rec[0] / Z64 - 1) <= 1e-6 and abs(rec[1] / kl64 - 1) <= 1e-6
    assert abs(rec[3] - Ph.astype(np.float64).sum()) <= 1e-6


def test_pca_column_means(gpu, monkeypatch):
    """HipPcaKernels.col_mean at (65, 3).  test_pca has no stored figure for this shape, so the gate is derived: the device adds the 65
    fp32 values of a column in float64, in some fixed order; any order of N - 1 float64 additions and the division by N are within
    N 2^-53 of the exact mean, relative to the column's mean absolute value.  Bit equality of the two runs is not claimed: the suite
    asserts it nowhere for slic_col_stats, and both runs pass the gate."""
    import tsne_ref as R
    from video_similarity_search_amd.decomposition import HipPcaKernels
    lib = _lib().load()
    N, D = 65, 3
    X = R.decaying(N, D, 0.85, 900 + N)
    ref = X.astype(np.float64).sum(axis=0) / N
    bound = N * 2.0 ** -53 * np.abs(X.astype(np.float64)).mean(axis=0)
    for mean, ws in run_both(monkeypatch, lambda: HipPcaKernels().col_mean(torch.from_numpy(X).cuda())):
        _only(ws, "pca_cs", lib.slic_col_stats_workspace_bytes(N, D))
        print("PCA column means off by", np.abs(mean - ref), "bound", bound)
        assert mean.dtype == np.float64 and mean.shape == (D,) and (np.abs(mean - ref) <= bound).all()


# =================================================================================================== clip transforms (tag `cliptf`)

@pytest.mark.parametrize("name", ["jitter_s0", "bench_s30"])
def test_clip_transforms(gpu, monkeypatch, name):
    """the two smallest golden inputs of clip_transforms_cases.py whose chain reaches the workspace (it holds the per-frame means of a
    contrast op; a chain without one asks for none): "fs" (3 x 2 x 5 x 7 floats) under ColorJitter and "us" (2 x 9 x 11 x 3 bytes) under
    the bench chain"""
    import clip_transforms_cases as cases
    from test_clip_transforms_gpu import G, close, seed
    from video_similarity_search_amd.coclr_utils import transforms as T
    lib = _lib().load()
    _, key, s, kind, build = [c for c in cases.CASES if c[0] == name][0]

    def run():
        seed(s)
        out = cases.run_case(build, T, T.Compose, T.Lambda, key, G[f"in_{key}"], device="cuda")
        assert (random.random(), np.random.uniform()) == tuple(G[f"next_{name}"])
        return out

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    n, ho, wo = b.shape[-3:]
    for ws in (wa, wb):
        _only(ws, "cliptf", lib.slic_clip_transform_workspace_bytes(1, n, ho, wo))
    assert torch.equal(a, b)                                                             # test_two_runs_are_bit_equal
    assert b.is_cuda and b.is_contiguous()
    close(name, b, G[f"out_{name}"], kind, G[f"dev_{name}"])


# =================================================================================================== k-means through kmeans_hip (tags km_*, kpp_*)

def _kmeans_rows(N, D, K):
    return np.random.default_rng(N + D + K).standard_normal((N, D)).astype(np.float32)


def _replay_kpp(Xc, picks, first, u, tol):
    """follow ONE k-means++ run's DEVICE picks in float64 (as test_g3_replay follows the device's OPTICS ordering): the first pick is the
    drawn row; every later pick is a row one of the step's draws can land on when cumulative sums move by at most tol, and its potential
    is, within 2 tol, no larger than the largest a candidate of SOME draw can have — what the argmin over the step's candidates
    guarantees whichever of the rows within tol the draws took.  Rows already at distance zero are not landed on."""
    x = Xc.astype(np.float64)
    N = len(x)

    def dist(r):
        return ((x - x[r]) ** 2).sum(1)

    assert picks[0] == first
    closest = dist(first)
    for c in range(1, len(picks)):
        pot = closest.sum()
        cs = np.cumsum(closest)
        v = u[c - 1] * pot
        lo = np.clip(np.searchsorted(cs, v - tol), None, N - 1)
        hi = np.clip(np.searchsorted(cs, v + tol), None, N - 1)
        sets = [[r for r in range(int(l), int(h) + 1) if closest[r] > 0 or r == l] for l, h in zip(lo, hi)]
        p = int(picks[c])
        assert any(p in s for s in sets), (c, p, sets)
        new_pot = {r: np.minimum(closest, dist(r)).sum() for s in sets for r in s}
        assert new_pot[p] <= min(max(new_pot[r] for r in s) for s in sets) + 2 * tol, (c, p)
        closest = np.minimum(closest, dist(p))


@pytest.mark.parametrize("N,D,K,R,precision", [(5, 16, 1, 1, None), (5, 16, 1, 3, None), (257, 8, 3, 1, None), (257, 8, 3, 3, None),
                                               (130, 40, 129, 1, None), (130, 40, 129, 3, None), (257, 8, 3, 1, "bf16")])
def test_kmeans_fit(gpu, monkeypatch, N, D, K, R, precision):
    """one fit with k-means++ seeding, single (slic_kmeanspp_run) and lock-step (slic_kmeanspp_run_batch, R = 3), fp32 and with the
    bf16 E-step forced.  Seeding: the draws of the fit's RandomState are made again on the host and every run's device picks are
    followed in float64 (_replay_kpp).  tol: an fp32 squared distance in the matrix form is off by at most (Dp + 2) 2^-24 (|x|^2 + |c|^2)
    (the bound csrc/dbscan.hip uses for an fp32 score), a potential or cumulative sum adds at most N of them, doubled as there:
    tol = 4 N (Dp + 2) 2^-24 max |x|^2.  Lloyd: the product's own host loop on the oracle provider (tests/kmeans_cpu_kernels.py), started
    from the rows the device picked — the same labels, iteration count and centres, inertia to 1e-12
    (test_fit_matches_oracle_and_golden's gate)."""
    import kmeans_cpu_kernels as ck
    from oracle import kmeans as okm
    from video_similarity_search_amd.clustering import KMeans
    from video_similarity_search_amd.clustering.kmeans_hip import _kpp_trials
    lib = _lib().load()
    X = _kmeans_rows(N, D, K)
    seed = 3
    Dp, T = (D + 7) // 8 * 8, _kpp_trials(K)

    def run():
        return KMeans(n_clusters=K, n_init=R, random_state=seed, precision=precision).fit(torch.from_numpy(X).cuda())

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    step, assign = ("km_step_bf16", "km_assign_bf16") if precision == "bf16" else ("km_step", "km_assign")
    want = {"km_cs": lib.slic_col_stats_workspace_bytes(N, Dp), "km_sum": lib.slic_sum_f32_to_f64_workspace_bytes(N),
            "km_step": lib.slic_kmeans_lloyd_step_workspace_bytes(N, K), "km_assign": lib.slic_kmeans_assign_workspace_bytes(N, K),
            "km_step_bf16": lib.slic_kmeans_lloyd_step_bf16_workspace_bytes(N, K),
            "km_assign_bf16": lib.slic_kmeans_assign_bf16_workspace_bytes(N, K),
            "kpp_run": lib.slic_kmeanspp_run_workspace_bytes(N, T), "kpp_batch": lib.slic_kmeanspp_run_batch_workspace_bytes(N, T, R)}
    for m, ws in ((a, wa), (b, wb)):
        for tag, nbytes in ws.log:
            assert tag in want and nbytes == want[tag], (tag, nbytes, want.get(tag))
        need = {"km_cs", "km_sum", step, "kpp_batch" if R > 1 else "kpp_run"}
        assert need <= ws.tags() <= need | {assign}, ws.tags()
        assert (assign in ws.tags()) or m.strict_                            # a run that stopped on tol relabels through the assign call
        assert (m.bf16_stats_ is not None) == (precision == "bf16")
    assert _same_bits(a.labels_, b.labels_) and a.inertia_ == b.inertia_ and a.n_iter_ == b.n_iter_
    assert _same_bits(a.cluster_centers_, b.cluster_centers_)
    picks = np.stack(b.init_indices_log_)
    assert picks.shape == (R, K) and _same_bits(picks, np.stack(a.init_indices_log_))
    Xc = X - okm.col_mean(X)
    tol = 4.0 * N * (Dp + 2) * 2.0 ** -24 * float((Xc.astype(np.float64) ** 2).sum(1).max())
    rs = np.random.RandomState(seed)
    for r in range(R):                                                           # KMeans._kmeans_plusplus.draw, run by run
        first = int(rs.choice(N, p=np.full(N, 1.0 / N)))
        u = rs.uniform(size=(K - 1, T)) if K > 1 else np.zeros((0, T))
        assert len(set(picks[r].tolist())) == K
        _replay_kpp(Xc, picks[r], first, u, tol)
    print((N, D, K, R), precision, "picks follow the float64 replay within", tol)
    ref = KMeans(n_clusters=K, init=[X[p] for p in picks], kernels=ck.OracleKernels()).fit(torch.from_numpy(X))
    assert np.array_equal(b.labels_, ref.labels_) and b.labels_.dtype == np.int32
    assert b.n_iter_ == ref.n_iter_ and b.strict_ == ref.strict_
    np.testing.assert_allclose(b.cluster_centers_, ref.cluster_centers_, rtol=0, atol=0)
    assert b.inertia_ == pytest.approx(ref.inertia_, rel=1e-12)


# =================================================================================================== convolution (tags `wgrad`, `splitk`)

def _conv_rules():
    return {
        "slic_conv_wgrad": lambda lib, a: lib.slic_conv_wgrad_workspace_bytes(a[0], a[3]),
        "slic_conv_wgrad_wino": lambda lib, a: lib.slic_conv_wgrad_wino_workspace_bytes(a[0], a[2]),
        "slic_conv_wgrad_wino2": lambda lib, a: lib.slic_conv_wgrad_wino2_workspace_bytes(a[0], a[2]),
        "slic_conv_gemm_tailsplit": lambda lib, a: lib.slic_conv_gemm_tailsplit_workspace_bytes(a[0], a[1], a[2], a[3]),
    }


def _bn_rules():
    return {
        "slic_bn_finalize": lambda lib, a: lib.slic_bn_finalize_workspace_bytes(a[1], a[3]),
        "slic_bn_bwd": lambda lib, a: lib.slic_bn_bwd_workspace_bytes(a[6], a[7], int(a[1] is not None and a[8] is None)),
        "slic_bn_bwd_fused": lambda lib, a: lib.slic_bn_bwd_fused_workspace_bytes(a[1], a[8]),
        "slic_bn_bwd_sums": lambda lib, a: lib.slic_bn_bwd_sums_workspace_bytes(a[7], a[8], a[1]),
    }


ENTRY_TAG = {"slic_conv_wgrad": "wgrad", "slic_conv_wgrad_wino": "wgrad", "slic_conv_wgrad_wino2": "wgrad", "slic_conv_gemm_tailsplit": "splitk",
             "slic_bn_finalize": "bn_fin", "slic_bn_bwd": "bn_bwd", "slic_bn_bwd_fused": "bn_bwd_fused", "slic_bn_bwd_sums": "bn_bwd_sums"}


def _spied_run(monkeypatch, poison, modules, rules, fn):
    """fn() under the guarded allocator with the library calls of `modules` recorded: every call that takes a workspace got a view of
    this allocator, under its tag, of exactly the bytes the query returns for the call's own arguments -> (outputs, entry points seen, ws)"""
    with guarded(monkeypatch, poison) as ws, spy_calls(monkeypatch, modules, rules) as seen:
        out = fn()
        ws.check()
    assert seen, "no library call that takes a workspace was made"
    for name, address, nbytes in seen:
        assert nbytes > 0 and ws.lookup(address) == (ENTRY_TAG[name], nbytes), (name, ws.lookup(address), nbytes)
    assert set(ws.tags()) == {ENTRY_TAG[name] for name, _, _ in seen}, (ws.tags(), seen)
    return out, [name for name, _, _ in seen], ws


WGRAD_CASES = [
    # kind, C, N, kernel, stride, pad, B, dims, entry point, gate (of max(1, |dW|_max)), bit-equal across the two runs
    ("direct", 8, 16, (3, 3, 3), (2, 2, 2), (1, 1, 1), 2, (8, 10, 10), "slic_conv_wgrad", 1e-4, False),
    ("wrun", 3, 8, (7, 7, 7), (1, 2, 2), (3, 3, 3), 2, (8, 20, 20), "slic_conv_wgrad", 1e-4, False),
    ("wino", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 2, (2, 4, 1), "slic_conv_wgrad_wino", 1e-4, True),
    ("wino", 128, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 3, (2, 5, 7), "slic_conv_wgrad_wino", 1e-4, True),
    ("wino2", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 2, (4, 8, 8), "slic_conv_wgrad_wino2", 2e-5, True),
]


@pytest.mark.parametrize("splits", [None, 3])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "{}_{}x{}".format(c[0], c[1], c[2]))
def test_conv_wgrad(gpu, monkeypatch, case, splits):
    """ConvPlan.wgrad against float64 F.conv3d autograd at test_conv_fwd_dgrad_wgrad's 1e-4 (the two-dimensional Winograd plan at
    test_conv_winograd_2d's own 2e-5).  The two Winograd weight gradients are bit-equal across the poisons, as their tests assert run to
    run; the direct and W-run kernels are held to the gate in both runs: the suite asserts no run-to-run bit equality for slic_conv_wgrad."""
    from test_encoder_gpu import _ndhwc
    from video_similarity_search_amd.models import conv_plan
    from video_similarity_search_amd.models.conv_plan import ConvPlan
    kind, C, N, k, s, p, B, dims, entry, gate, bit_equal = case
    rng = np.random.default_rng(C * 7 + N)
    x = torch.from_numpy(rng.standard_normal((B, C) + dims).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((N, C) + k) / np.sqrt(C * np.prod(k))).astype(np.float32))
    x64, w64 = x.double(), w.double().requires_grad_(True)
    y64 = F.conv3d(x64, w64, None, s, p)
    dy = torch.from_numpy(rng.standard_normal(tuple(y64.shape)).astype(np.float32))
    gw64, = torch.autograd.grad(y64, [w64], dy.double())
    if kind == "direct":
        plan = ConvPlan(C, N, k, s, p, dims, "cuda", wrun=False, wino=False)
        xd = _ndhwc(x, plan.Cs).cuda()
    elif kind == "wrun":
        plan = ConvPlan(C, N, k, s, p, dims, "cuda")
        assert plan.wrun
        xd = plan.make_source(x.cuda())
    elif kind == "wino":
        plan = ConvPlan(C, N, k, s, p, dims, "cuda", wino=True, wino2=False, wino2_wgrad=False)
        assert plan.wino_wgrad and not plan.wino2_wgrad
        xd = _ndhwc(x, C).cuda()
    else:
        plan = ConvPlan(C, N, k, s, p, dims, "cuda", wino=True, wino2=True, wino2_wgrad=True)
        assert plan.wino2_wgrad
        xd = _ndhwc(x, C).cuda()
    wd = w.cuda().contiguous()
    dyd = dy.permute(0, 2, 3, 4, 1).contiguous().cuda()
    outs = []
    for poison in (0x00, 0xFF):
        dW, names, _ = _spied_run(monkeypatch, poison, [conv_plan], _conv_rules(),
                                  lambda: plan.wgrad(xd, dyd, B, torch.full_like(wd, float("nan")), splits=splits).cpu())
        assert names == [entry], names
        err = (dW - gw64.float()).abs().max().item()
        print(kind, (C, N, B, dims), "splits", splits, "max |dW - dW64|", err, "gate", gate * max(1.0, gw64.abs().max().item()))
        assert err <= gate * max(1.0, gw64.abs().max().item())
        outs.append(dW)
    if bit_equal:
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("variant,slots,want", [(20, 8, (4, 4)), (22, 4, (2, 2))])
def test_conv_tailsplit_forward(gpu, monkeypatch, variant, slots, want):
    """the tail-split forward of test_conv_tailsplit_matches_single_pass against float64 F.conv3d at test_conv_fwd_dgrad_wgrad's forward
    tolerance, the ReLU / addend epilogue at four times it as the Winograd tests take it.  Bit equality of the two runs is not claimed:
    the suite compares the split launch with the one-pass one by allclose only."""
    from video_similarity_search_amd.models import conv_plan
    from video_similarity_search_amd.models.conv_plan import ConvPlan
    rng = np.random.default_rng(5)
    C, N, B, dims = 256, 128, 3, (2, 7, 7)
    plan = ConvPlan(C, N, (3, 3, 3), (1, 1, 1), (1, 1, 1), dims, "cuda", wino=False)
    xh = rng.standard_normal((B,) + dims + (C,)).astype(np.float32)
    wh = (rng.standard_normal((N, C, 3, 3, 3)) / np.sqrt(C * 27)).astype(np.float32)
    rh = rng.standard_normal((B,) + dims + (N,)).astype(np.float32)
    x, w, res = (torch.from_numpy(t).cuda() for t in (xh, wh, rh))
    y64 = F.conv3d(torch.from_numpy(xh).double().permute(0, 4, 1, 2, 3), torch.from_numpy(wh).double(), None, 1, 1).permute(0, 2, 3, 4, 1)
    r64 = F.relu(y64 + torch.from_numpy(rh).double())
    tol = 2e-6 * np.sqrt(C * 27) + 1e-6
    wp = plan.pack_fwd(w)
    monkeypatch.setenv("SLIC_CONV_TAIL", "1")
    monkeypatch.setenv("SLIC_CONV_TAIL_SLOTS", str(slots))
    assert plan._plan_split(plan._fwd_args(x, B), variant) == want

    def run():
        z, _ = plan.forward(x, wp, B, want_stats=True, variant=variant)
        y, _ = plan.forward(x, wp, B, addend=res, relu=True, variant=variant)
        return z.cpu().double(), y.cpu().double()

    for poison in (0x00, 0xFF):
        (z, y), names, _ = _spied_run(monkeypatch, poison, [conv_plan], _conv_rules(), run)
        assert names == ["slic_conv_gemm_tailsplit"] * 2
        ez, ey = (z - y64).abs().max().item(), (y - r64).abs().max().item()
        print("tail split", variant, want, "max |z - z64|", ez, "gate", tol * max(1.0, y64.abs().max().item()), "epilogue", ey)
        assert ez <= tol * max(1.0, y64.abs().max().item())
        assert ey <= 4 * tol * max(1.0, r64.abs().max().item())


# =================================================================================================== engine (tags bn_*)

def test_engine_train_step(gpu, monkeypatch, golden_dir):
    """one train step of the tiny encoder against tests/golden/encoder_tiny.npz under the gates of
    test_tiny_encoder_train_step_vs_reference_golden (literals in that test's body: embeddings and loss 1e-4, every gradient
    1e-6 + 5e-4 of its tensor's largest entry).  In the four bn_* tags the Python side chooses the size arguments, so every library call
    is held to the query for its own arguments.  Bit equality of the two runs is not claimed: the suite asserts it for no whole step."""
    from test_encoder_gpu import R3D18_KW, _load_into
    from video_similarity_search_amd.loss import OnlineTripletLoss
    from video_similarity_search_amd.models import conv_plan, generate_model, resnet
    enc = dict(np.load(os.path.join(golden_dir, "encoder_tiny.npz")))
    sd = {k[3:]: v for k, v in enc.items() if k.startswith("sd/")}
    x = torch.from_numpy(enc["x"]).cuda()

    def run():
        m = generate_model(18, **dict(R3D18_KW, widen_factor=0.125, hidden_layer=64, out_dim=32))
        _load_into(m, sd)
        m = m.cuda().train()
        emb = m(x)
        loss, _ = OnlineTripletLoss(0.2, 'cosine')(emb, torch.arange(2).repeat(2).cuda(), sampling_strategy='noise_contrastive')
        loss.backward()
        return emb.detach().cpu().numpy(), loss.item(), {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}

    rules = dict(_conv_rules(), **_bn_rules())
    for poison in (0x00, 0xFF):
        (emb, loss, grads), names, ws = _spied_run(monkeypatch, poison, [conv_plan, resnet], rules, run)
        print("engine step: workspace tags", sorted(ws.tags()), "calls", {n: names.count(n) for n in sorted(set(names))})
        assert "bn_fin" in ws.tags() and ws.tags() & {"bn_bwd", "bn_bwd_sums", "bn_bwd_fused"}
        np.testing.assert_allclose(emb, enc["train/emb"], atol=1e-4, rtol=0)
        assert abs(loss - float(enc["train/loss"])) < 1e-4
        for k, g in grads.items():
            ref = enc["grad/" + k]
            np.testing.assert_allclose(g, ref, atol=1e-6 + 5e-4 * np.abs(ref).max(), rtol=0, err_msg=k)


# =================================================================================================== MoCo (tag `moco`, sized in Python)

def test_moco_constants_mirror_the_header():
    import re
    from conftest import ROOT
    from video_similarity_search_amd.loss import NCE_loss
    text = open(os.path.join(ROOT, "include", "slic_hip.h")).read()
    parts = {n: int(v) for n, v in re.findall(r"#define\s+(SLIC_MOCO_(?:DQ_)?PARTS)\s+(\d+)", text)}
    assert (NCE_loss._MOCO_PARTS, NCE_loss._MOCO_DQ_PARTS) == (parts["SLIC_MOCO_PARTS"], parts["SLIC_MOCO_DQ_PARTS"])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("B,D,K", [(1, 100, 1000), (5, 3, 130), (26, 128, 2048)])
def test_moco(gpu, monkeypatch, B, D, K, fused):
    """MemoryMoCo, one step, against the float64 provider under gates_at of test_moco_gpu.py (test_against_float64_fused_and_unfused)"""
    from test_moco_gpu import dev, gates_at, module, unit
    from video_similarity_search_amd.loss.NCE_loss import _MOCO_DQ_PARTS, _MOCO_PARTS, NCESoftmaxLoss
    rng = np.random.default_rng(B * 1000 + D)
    q, k, mem = unit(rng, B, D), unit(rng, B, D), unit(rng, K, D)
    (x64, l64, dq64), (g_x, g_l, g_dq) = gates_at(q, k, mem)
    start = K - B // 2 if B > 1 else K - 1                                    # the enqueue wraps

    def run():
        m = module(K, D, mem)
        m.index = start
        qd = dev(q).requires_grad_(True)
        out = None
        if fused:
            loss = m.softmax_loss(qd, dev(k))
        else:
            out = m(qd, dev(k))
            loss = NCESoftmaxLoss()(out)
        loss.backward()
        return (None if out is None else out.detach().cpu().numpy()), loss.detach().cpu().numpy(), qd.grad.cpu().numpy(), \
            m.memory.cpu().numpy(), m.index

    (a, wa), (b, wb) = run_both(monkeypatch, run)
    bwd = ("moco", _MOCO_DQ_PARTS * B * D * 4)
    for ws in (wa, wb):
        assert ws.log == ([("moco", _MOCO_PARTS * B * 16), bwd] if fused else [bwd]), ws.log
    assert all(x is None and y is None or _same_bits(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]     # test_two_runs_are_bit_equal
    out, loss, dq, memory, index = b
    e_dq = np.abs(dq - dq64).max() / np.abs(dq64).max()
    print((B, D, K), "fused" if fused else "unfused", "loss", abs(float(loss) - l64) / l64, "/", g_l, "dq", e_dq, "/", g_dq)
    if out is not None:
        print("logits", np.abs(out - x64).max(), "/", g_x)
        assert np.abs(out - x64).max() <= g_x
    assert abs(float(loss) - l64) <= g_l * l64 and e_dq <= g_dq
    expect = mem.copy()
    expect[(start + np.arange(B)) % K] = k
    assert index == (start + B) % K and np.array_equal(memory, expect)


# =================================================================================================== coclr_classify (tag `classify_cs`)

def test_classify_centre(gpu, monkeypatch):
    """HipClassifyKernels.centre on 6 x 21 features, the test-set shape of test_test_retrieval_against_float64_sort (21 columns: padded
    to 24).  Derived gate: the mean is a float64 sum rounded once to fp32 and the subtraction rounds once, so an entry is within
    2^-24 (|mean| + |x - mean|) of the float64 centring, and the float64 sum itself within N 2^-53 mean|x|.  Bit equality of the two
    runs is not claimed: the suite asserts it nowhere for slic_col_stats; both runs pass the gate."""
    from video_similarity_search_amd import coclr_classify as cc
    lib = _lib().load()
    N, D = 6, 21
    X = (np.random.default_rng(41).standard_normal((N, D)) + 0.5).astype(np.float32)
    x64 = X.astype(np.float64)
    mean = x64.mean(axis=0)
    ref = x64 - mean
    bound = 2.0 ** -24 * (np.abs(mean)[None, :] + np.abs(ref)) * (1 + 2.0 ** -20) + N * 2.0 ** -53 * np.abs(x64).mean(axis=0)[None, :]
    for out, ws in run_both(monkeypatch, lambda: cc.HipClassifyKernels().centre(torch.from_numpy(X).cuda()).cpu().numpy()):
        _only(ws, "classify_cs", lib.slic_col_stats_workspace_bytes(N, 24))
        err = np.abs(out.astype(np.float64) - ref)
        print("centre: worst error / bound", (err / bound).max())
        assert out.shape == (N, D) and (err <= bound).all()
